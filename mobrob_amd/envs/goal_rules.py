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


HAZARD_FRAMES_MAX_BYTES = 64 << 20   # cap on a MovingHazards table (S * F * M * 12 bytes); the engine refuses a larger one too


class MovingHazards:
    """Hazards that move: `Hazards` plus a time axis of F piecewise-constant FRAMES.  `locations` [F, M, 2] (one scene) or
    [S, F, M, 2], `size` a scalar, [M], [S, M] or [S, F, M]; `frame_steps` >= 1 steps per frame; `loop`: wrap around after the
    last frame instead of holding it; `counts` [S] (constant over the frames), `scene`, `cost`, `indicator` as for `Hazards`.
    The table is float32 [S, F, M, 3].  Checked on construction (ValueError).

    Time: the check after a robot's step with 0-based GLOBAL step number g uses frame
        f(g) = min(g // frame_steps, F - 1)   (hold the last frame)        or, with loop,   f(g) = (g // frame_steps) % F.
    In a waypoint-following run g = step0 + t; in an evaluation g = t, the step of the call (episode resets do not reset the
    clock).  Cost and clearance at that frame are `hazard_cost` of the frame's rows: nothing is interpolated."""

    def __init__(self, locations, size=HAZARDS_SIZE, frame_steps=1, loop=False, cost=HAZARDS_COST, indicator=True, counts=None,
                 scene=None):
        loc = np.asarray(locations, np.float64)
        if loc.ndim == 3:
            loc = loc[None]
        if loc.ndim != 4 or loc.shape[3] != 2:
            raise ValueError(f"moving hazard locations must be [F, M, 2] or [S, F, M, 2], got shape {np.shape(locations)}")
        S, F, M = loc.shape[:3]
        if S < 1:
            raise ValueError("hazards need at least one scene")
        if F < 1:
            raise ValueError("moving hazards need at least one frame")
        if M > HAZARDS_MAX:
            raise ValueError(f"at most {HAZARDS_MAX} hazards per scene, got {M}")
        if S * F * M * 12 > HAZARD_FRAMES_MAX_BYTES:
            raise ValueError(f"hazard frames of {S} x {F} x {M} x 12 bytes exceed the cap of {HAZARD_FRAMES_MAX_BYTES} bytes "
                             f"({HAZARD_FRAMES_MAX_BYTES >> 20} MiB)")
        if isinstance(frame_steps, bool) or not isinstance(frame_steps, (int, np.integer)) or frame_steps < 1:
            raise ValueError(f"frame_steps must be an integer >= 1, got {frame_steps!r}")
        if frame_steps > 2 ** 31 - 1:
            raise ValueError("frame_steps must fit an int32")
        rad = np.asarray(size, np.float64)
        if rad.shape not in ((), (M,), (S, M), (S, F, M)):
            raise ValueError(f"hazard size must be a scalar, [{M}], [{S}, {M}] or [{S}, {F}, {M}], got shape {rad.shape}")
        rad = np.broadcast_to(rad[:, None, :] if rad.shape == (S, M) else rad, (S, F, M))
        if not (np.all(np.isfinite(loc)) and np.all(np.isfinite(rad))):
            raise ValueError("hazard locations and sizes must be finite")
        if np.any(rad < 0):
            raise ValueError("hazard sizes must be >= 0")
        static = Hazards(np.zeros((S, M, 2)), 0.0, cost, indicator, counts, scene)   # cost, counts and scene: Hazards' checks
        self.table = np.ascontiguousarray(np.concatenate([loc, rad[..., None]], axis=-1), np.float32)   # [S, F, M, 3]
        self.counts, self.scene, self.cost, self.indicator = static.counts, static.scene, static.cost, static.indicator
        self.frame_steps, self.loop = int(frame_steps), bool(loop)

    @property
    def n_scenes(self):
        return self.table.shape[0]

    @property
    def n_frames(self):
        return self.table.shape[1]

    @property
    def max_hazards(self):
        return self.table.shape[2]

    def frame_index(self, step):
        """The frame in force at the check after the step with 0-based global number `step`."""
        step = int(step)
        if step < 0:
            raise ValueError("step must be >= 0")
        k = step // self.frame_steps
        return k % self.n_frames if self.loop else min(k, self.n_frames - 1)

    def rows(self, robot=0, step=0):
        """[m, 3] (x, y, radius) float64 of the hazards robot `robot` sees at the check after global step `step` (the float32
        values the device uses)."""
        s = 0 if self.scene is None else int(self.scene[robot])
        return self.table[s, self.frame_index(step), : self.counts[s]].astype(np.float64)

    check_robots = Hazards.check_robots

    @staticmethod
    def circling_offsets(travel, n_frames, dt, phase0=0.0):
        """[n_frames, 2] float64: the reference Engine's gremlin motion (engine.py set_mocaps, gremlins_travel): at simulation
        time phi the gremlin sits at travel * (sin phi, cos phi); frame j is taken at phi = phase0 + j * dt."""
        out = np.zeros((int(n_frames), 2))
        for j in range(int(n_frames)):
            phase = float(phase0 + j * dt)
            out[j] = np.array([np.sin(phase), np.cos(phase)]) * travel
        return out

    @classmethod
    def circling(cls, centres, travel=0.3, size=0.1, n_frames=1, dt=0.05, phase0=0.0, **kwargs):
        """Hazards circling as the reference's gremlins do: frame j holds centres + circling_offsets(...)[j], computed in
        float64 and stored as float32.  centres [M, 2] or [S, M, 2]; travel: the circle's radius (gremlins_travel 0.3), size
        the hazard radius (gremlins_size 0.1), dt the simulation time per frame (with frame_steps = 1: the env's dt).  With
        n_frames * dt = 2 pi and loop=True the motion is periodic.  The offset rule is the reference's (pinned by
        tests/golden/gremlin_cases.npz); adding a placement centre to it is this project's: the reference moves a mocap body
        whose pose MuJoCo composes with the placement.  kwargs: frame_steps, loop, cost, indicator, counts, scene."""
        c = np.asarray(centres, np.float64)
        if c.ndim == 2:
            c = c[None]
        if c.ndim != 3 or c.shape[2] != 2:
            raise ValueError(f"centres must be [M, 2] or [S, M, 2], got shape {np.shape(centres)}")
        if int(n_frames) < 1:
            raise ValueError("moving hazards need at least one frame")
        if not (np.isfinite(travel) and np.isfinite(dt) and np.isfinite(phase0)):
            raise ValueError("travel, dt and phase0 must be finite")
        off = cls.circling_offsets(float(travel), n_frames, float(dt), float(phase0))
        loc = c[:, None, :, :] + off[None, :, None, :]
        return cls(loc if np.ndim(centres) == 3 else loc[0], size, **kwargs)


# ---- teams: pairwise separation costs between the robots of a waypoint-following run.  This project's own rule (the reference
# has one robot per world); it is stated here once and the device (csrc/kernels_team.h) and the host loop are held to it.
TEAM_SIZES = (1, 2, 4, 8, 16)   # they divide 16: a team never straddles a tile of the device kernel
TEAM_START = (0.0, 0.0, -1.0, np.nan, -1.0)   # a robot's team record before its first step


class Teams:
    """Robots partitioned into teams of `size` consecutive robots (team of robot n: n // size, team-local index n % size) that
    must keep `separation` apart: `cost` per unit of intrusion, `indicator`: a step's cost is 1 if there is any.  Robots of
    different teams never see each other.  Checked on construction (ValueError).  `solid`: False -- the mates are observed
    (team_cost) and block nothing; True -- a waypoint-following run also resolves every step against the mates (team_block):
    a robot stops or slides at the square of half-width `separation` around each mate."""

    def __init__(self, size, separation, cost=1.0, indicator=False, solid=False):
        if isinstance(size, bool) or not isinstance(size, (int, np.integer)) or int(size) not in TEAM_SIZES:
            raise ValueError(f"team size must be one of {TEAM_SIZES}, got {size!r}")
        separation, cost = float(separation), float(cost)
        if not np.isfinite(separation) or separation < 0:
            raise ValueError(f"team separation must be finite and >= 0, got {separation}")
        if not np.isfinite(cost) or cost < 0:
            raise ValueError(f"team cost must be finite and >= 0, got {cost}")
        self.size, self.indicator = int(size), bool(indicator)
        self.separation, self.cost = float(np.float32(separation)), float(np.float32(cost))   # the float32 values every path uses
        self.solid = bool(solid)

    def check_robots(self, n):
        if int(n) % self.size != 0:
            raise ValueError(f"{int(n)} robots do not split into teams of {self.size}")


def team_cost(pos_xy, stepped, separation, coef=1.0, indicator=False):
    """The team check of ONE step: pos_xy [..., G, 2] the post-step x, y of the G members of a team (a member that did not step:
    where it stands), stepped [..., G] who stepped -> (cost [..., G] float32, clear [..., G] float32, partner_local [..., G]
    int64) for the members that stepped; the others get 0, +inf, -1 and account nothing.  Leading dimensions are teams (or
    steps) handled alike.  For member i and its mates j != i:
        d_ij = |p_i - p_j|      cost_i = coef * sum over d_ij <= separation of (separation - d_ij)      indicator: cost_i > 0
        clear_i = min_j (d_ij - separation)  (+inf alone)      partner_i = the j attaining it (equal clearances: the lowest j)
    in float32, every operation rounded on its own, in the device's order: four partial sums, quarter q over the members
    m = q, q + 4, ... except i, combined as (p0 + p1) + (p2 + p3), coef applied once afterwards; the (clearance, partner) minimum
    over the same quarters and exchanges, the smaller clearance winning and equal clearances going to the smaller index.
    d_ij == separation contributes exactly 0."""
    f32 = np.float32
    p = np.asarray(pos_xy, f32)
    stepped = np.asarray(stepped, bool)
    G = p.shape[-2]
    if p.shape[-1] != 2 or stepped.shape != p.shape[:-1]:
        raise ValueError(f"pos_xy must be [..., G, 2] and stepped [..., G], got {p.shape} and {stepped.shape}")
    sep, lead = f32(separation), p.shape[:-2]
    me = np.arange(G)
    part, clear, partner = np.zeros((4,) + lead + (G,), f32), np.full((4,) + lead + (G,), np.inf, f32), np.full((4,) + lead + (G,), -1)
    for m in range(G):
        q = m % 4
        dx, dy = p[..., :, 0] - p[..., m:m + 1, 0], p[..., :, 1] - p[..., m:m + 1, 1]
        d = np.sqrt(dx * dx + dy * dy)                                    # float32 throughout: each operation correctly rounded
        other = me != m
        part[q] = np.where(other & (d <= sep), part[q] + (sep - d), part[q])
        cl = d - sep
        closer = other & (cl < clear[q])                                  # ascending m: equal clearances keep the lower index
        clear[q], partner[q] = np.where(closer, cl, clear[q]), np.where(closer, m, partner[q])

    def closer_of(a, b):
        (ca, pa), (cb, pb) = a, b
        take = (cb < ca) | ((cb == ca) & (pb < pa))
        return np.where(take, cb, ca), np.where(take, pb, pa)
    total = f32(coef) * ((part[0] + part[1]) + (part[2] + part[3]))
    cl, pt = closer_of(closer_of((clear[0], partner[0]), (clear[1], partner[1])), closer_of((clear[2], partner[2]), (clear[3], partner[3])))
    if indicator:
        total = (total > 0).astype(f32)
    return (np.where(stepped, total, f32(0)), np.where(stepped, cl, f32(np.inf)).astype(f32), np.where(stepped, pt, -1).astype(np.int64))


def team_fold(record, pos_xy, stepped, teams, step0=0):
    """The carried team record after the steps step0 .. step0 + T - 1: record [n][5] float64 (sum of step costs, steps with
    cost > 0, the first such step as a global 1-based number or -1, the minimum clearance over the run -- NaN before the robot's
    first step, +inf in a team of one --, the partner's global index at that minimum, first attainment kept, or -1), pos_xy
    [T][n][2] the positions after each step (a robot that did not step: where it stands), stepped [T][n].  Returns a new
    [n][5]; a robot accounts only for the steps in which it stepped itself."""
    rec = np.array(record, np.float64)
    pos = np.asarray(pos_xy, np.float32)
    stepped = np.asarray(stepped, bool)
    T, n = stepped.shape
    teams.check_robots(n)
    if rec.shape != (n, 5) or pos.shape != (T, n, 2):
        raise ValueError(f"record must be [{n}][5] and pos_xy [{T}][{n}][2], got {rec.shape} and {pos.shape}")
    G = teams.size
    cost, clear, partner = team_cost(pos.reshape(T, n // G, G, 2), stepped.reshape(T, n // G, G), teams.separation, teams.cost,
                                     teams.indicator)
    cost, clear = cost.reshape(T, n).astype(np.float64), clear.reshape(T, n).astype(np.float64)
    partner = np.where(partner < 0, -1, partner + (np.arange(n // G) * G)[None, :, None]).reshape(T, n)
    for t in range(T):
        s = stepped[t]
        rec[:, 0] += np.where(s, cost[t], 0.0)                            # float64, one step after the other
        hit = s & (cost[t] > 0)
        rec[:, 1] += hit
        rec[:, 2] = np.where(hit & (rec[:, 2] < 0), step0 + t + 1, rec[:, 2])
        best = np.where(np.isnan(rec[:, 3]), np.inf, rec[:, 3])
        closer = s & (clear[t] < best)
        rec[:, 3] = np.where(s, np.where(closer, clear[t], best), rec[:, 3])
        rec[:, 4] = np.where(closer, partner[t], rec[:, 4])
    return rec


# ---- timed waypoints: release steps and holds in a waypoint-following run.  This project's own rule; it is stated here once and
# the device (csrc/kernels_follow.h: ScheduledFollowTask) and the host loop are held to it.
SCHED_START = (0.0, np.nan)   # a robot's hold record before its first hold step


class Schedule:
    """Release steps for the waypoints of a run: `release` [n][K] (or [K], the same for every robot) integers >= 0, `home` [n][P]
    finite (None: the robots' starts, filled in by FollowState).  Waypoint k of robot i may not be the goal in force in a step
    whose 0-based GLOBAL number g is below release[i][k]; until then the robot holds at its anchor, under the policy:
        holding(k, g) = k < n_waypoints[i] and g < release[i][k]
        anchor(k)     = waypoints[i][k - 1] if k > 0 else home[i]
        goal(k, g)    = anchor(k) if holding(k, g) else waypoints[i][min(k, n_waypoints[i] - 1)]
    k is the robot's count of waypoints reached (the index of the waypoint it is on), so the goal of a step is a pure function of
    (k, g) and nothing is carried for it.  A release earlier than its predecessor's never holds.  Checked on construction
    (ValueError); entries past a robot's waypoint count are ignored."""

    def __init__(self, release, home=None):
        rel = np.asarray(release)
        if rel.ndim not in (1, 2) or rel.size == 0 or not np.issubdtype(rel.dtype, np.integer) or rel.dtype == bool:
            raise ValueError(f"release must be integers of shape [K] or [n, K], got {rel.dtype} of shape {rel.shape}")
        if np.any(rel < 0) or np.any(rel > 2 ** 31 - 1):
            raise ValueError("release steps must lie in 0 .. 2^31 - 1")
        self.release = np.ascontiguousarray(rel, np.int32)
        self.home = None
        if home is not None:
            h = np.asarray(home, np.float64)
            if h.ndim != 2 or not np.all(np.isfinite(h)):
                raise ValueError(f"home must be finite of shape [n, pos_dim], got shape {h.shape}")
            self.home = np.ascontiguousarray(h, np.float32)

    def for_robots(self, n, K, start=None):
        """-> (release [n][K] int32, home [n][P] float32) for a run of n robots with K waypoint slots; a missing home is `start`"""
        rel = self.release
        if rel.ndim == 1:
            rel = np.broadcast_to(rel, (n, rel.shape[0]))
        if rel.shape[0] != n or rel.shape[1] > K:
            raise ValueError(f"release must be [{n}, K'] or [K'] with K' <= {K}, got shape {self.release.shape}")
        out = np.zeros((n, K), np.int32)
        out[:, :rel.shape[1]] = rel
        home = self.home if self.home is not None else start
        if home is None or np.shape(home)[0] != n:
            raise ValueError(f"home must have {n} rows, one per robot")
        return out, np.ascontiguousarray(home, np.float32)

    @staticmethod
    def holding(release, n_waypoints, k, step):
        """[n] bool: does robot i, on waypoint k[i], hold in the step with global number `step` ([n] or a scalar)?"""
        release, nw, k = np.asarray(release), np.asarray(n_waypoints), np.asarray(k)
        kk = np.minimum(k, release.shape[1] - 1)
        return (k < nw) & (np.asarray(step) < release[np.arange(len(k)), kk])

    @staticmethod
    def goal(release, home, waypoints, n_waypoints, k, step):
        """[n][P]: the goal in force of every robot in the step with global number `step` (a robot without waypoints: NaN)"""
        wp, nw, k = np.asarray(waypoints), np.asarray(n_waypoints), np.asarray(k)
        rows = np.arange(len(k))
        hold = Schedule.holding(release, nw, k, step)
        on = wp[rows, np.clip(np.minimum(k, nw - 1), 0, None)]
        anchor = np.where((k > 0)[:, None], wp[rows, np.clip(k - 1, 0, None)], np.asarray(home, wp.dtype))
        out = np.where(hold[:, None], anchor, on)
        return np.where((nw > 0)[:, None], out, np.nan)

    @staticmethod
    def lateness(release, arrival):
        """[n][K] float64: arrival[k] - release[k] (global steps; an arrival is 1-based, so a robot released at g that needs one
        step is 1 late), NaN where the waypoint was not reached"""
        arrival = np.asarray(arrival)
        return np.where(arrival > 0, arrival.astype(np.float64) - np.asarray(release, np.float64), np.nan)


def _fma32(a, b, c):
    """float32 fma(a, b, c), correctly rounded: the product is exact in float64, the float64 sum is rounded to odd (TwoSum tells
    which way the exact value lies), and the final rounding to float32 is then the one of the exact value"""
    p, c = np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64), np.asarray(c, np.float32).astype(np.float64)
    s = p + c
    v = s - p
    err = (p - (s - v)) + (c - v)
    even = (np.ascontiguousarray(s).view(np.int64) & 1) == 0
    s = np.where((err != 0) & even, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def goal_distance32(goal, pos):
    """The device's goal_dist (csrc/kernels_env.h) bit for bit: float32 differences, the squares summed by fused multiply-adds in
    component order, the root taken in float64 and rounded once: [..., p], [..., p] -> [...] float32"""
    d = np.asarray(goal, np.float32) - np.asarray(pos, np.float32)
    s = np.zeros(d.shape[:-1], np.float32)
    for j in range(d.shape[-1]):
        s = _fma32(d[..., j], d[..., j], s)
    return np.sqrt(s.astype(np.float64)).astype(np.float32)


def schedule_fold(record, anchor, pos, held):
    """The carried hold record after the steps of a call: record [n][2] float64 (hold steps run, the largest distance to the
    anchor after a hold step -- NaN before the first), anchor [T][n][P] the goal in force in each step, pos [T][n][P] the
    positions after it (float32: the device's), held [T][n] the robot's hold steps.  Returns a new [n][2]: the count continued,
    the maximum of goal_distance32 taken in float32 step after step and widened."""
    rec = np.array(record, np.float64)
    held = np.asarray(held, bool)
    T, n = held.shape
    anchor, pos = np.asarray(anchor, np.float32), np.asarray(pos, np.float32)
    if rec.shape != (n, 2) or anchor.shape != pos.shape or pos.shape[:2] != (T, n):
        raise ValueError(f"record must be [{n}][2], anchor and pos [{T}][{n}][P], got {rec.shape}, {anchor.shape} and {pos.shape}")
    for t in range(T):
        h = held[t]
        d = goal_distance32(anchor[t], pos[t]).astype(np.float64)
        best = np.where(np.isnan(rec[:, 1]), 0.0, rec[:, 1])
        rec[:, 0] += h
        rec[:, 1] = np.where(h, np.maximum(best, d), rec[:, 1])
    return rec


# ---- walls: axis-aligned boxes in a waypoint-following run, checked for contact and for crossing.  The boxes are the reference's
# (its turtlebot3 arena is four of them, its Engine takes walls_locations / walls_size with rot 0); the checks are this project's
# own rule, stated here once, and the device (csrc/kernels_wall.h) and the host loop are held to it.
WALLS_MAX = 1024         # walls per scene the device path takes
WALL_START = (0.0, 0.0, -1.0, np.nan, -1.0, 0.0, -1.0)   # a robot's wall record before its first step
ARENA_LENGTH, ARENA_THICK = 2.42 + 0.28 * 2, 0.265       # the reference's turtlebot3 enclosure


class Walls:
    """A wall layout: `boxes` [M, 4] (one scene) or [S, M, 4] (scenes) rows (cx, cy, hx, hy) -- centre and half extents, hx, hy
    >= 0 --, `counts` [S] walls in use per scene (None: all M), `scene` [n] scene of each robot (None: S must be 1), `radius` the
    robot's footprint, `cost` per unit of intrusion and `indicator` (a step's cost is 1 if there is any).  Only x and y count,
    for every robot.  Checked on construction (ValueError).  `solid`: False -- the walls are observed (wall_check) and block
    nothing; True -- a waypoint-following run also resolves every step against them (wall_block): robots stop and slide."""

    def __init__(self, boxes, counts=None, scene=None, radius=0.0, cost=1.0, indicator=True, solid=False):
        bx = np.asarray(boxes, np.float64)
        if bx.size == 0 and bx.ndim < 2:
            bx = bx.reshape(0, 4)
        if bx.ndim == 2:
            bx = bx[None]
        if bx.ndim != 3 or bx.shape[2] != 4:
            raise ValueError(f"wall boxes must be [M, 4] or [S, M, 4], got shape {np.shape(boxes)}")
        S, M = bx.shape[:2]
        if S < 1:
            raise ValueError("walls need at least one scene")
        if M > WALLS_MAX:
            raise ValueError(f"at most {WALLS_MAX} walls per scene, got {M}")
        if not np.all(np.isfinite(bx)):
            raise ValueError("wall boxes must be finite")
        if np.any(bx[..., 2:] < 0):
            raise ValueError("wall half extents must be >= 0")
        radius, cost = float(radius), float(cost)
        if not np.isfinite(radius) or radius < 0:
            raise ValueError(f"robot radius must be finite and >= 0, got {radius}")
        if not np.isfinite(cost) or cost < 0:
            raise ValueError(f"wall cost must be finite and >= 0, got {cost}")
        if counts is None:
            cnt = np.full(S, M, np.int32)
        else:
            cnt = np.asarray(counts)
            if cnt.shape != (S,) or not np.issubdtype(cnt.dtype, np.integer) or np.any(cnt < 0) or np.any(cnt > M):
                raise ValueError(f"wall counts must be {S} integers in 0 .. {M}")
            cnt = cnt.astype(np.int32)
        if scene is None:
            if S != 1:
                raise ValueError(f"{S} wall scenes need a scene index per robot")
            sc = None
        else:
            sc = np.asarray(scene)
            if sc.ndim != 1 or not np.issubdtype(sc.dtype, np.integer) or np.any(sc < 0) or np.any(sc >= S):
                raise ValueError(f"wall scene indices must be integers in 0 .. {S - 1}")
            sc = sc.astype(np.int32)
        self.table = np.ascontiguousarray(bx, np.float32)   # [S, M, 4]
        self.counts, self.scene, self.indicator = cnt, sc, bool(indicator)
        self.radius, self.cost = float(np.float32(radius)), float(np.float32(cost))   # the float32 values every path uses
        self.solid = bool(solid)

    @property
    def n_scenes(self):
        return self.table.shape[0]

    @property
    def max_walls(self):
        return self.table.shape[1]

    def rows(self, robot=0):
        """[m, 4] float32 (cx, cy, hx, hy) of the walls robot `robot` sees"""
        s = 0 if self.scene is None else int(self.scene[robot])
        return self.table[s, : self.counts[s]]

    def check_robots(self, n):
        if self.scene is not None and self.scene.shape != (n,):
            raise ValueError(f"wall scene must have {n} entries, one per robot, got {self.scene.shape[0]}")

    @staticmethod
    def enclosure(length=ARENA_LENGTH, thick=ARENA_THICK, centre=(0.0, 0.0), solid=None, **kwargs):
        """With `solid` given (True or False): the Walls of the enclosure below, Walls(boxes, solid=solid, **kwargs).  Otherwise the
        [4, 4] float64 boxes of a square enclosure of outer side `length` and wall thickness `thick` around `centre`, laid out
        as the reference's arena is (pinned by tests/golden/wall_cases.npz): four equal bars in a pinwheel, each reaching from one
        outer corner to the inner face of the next bar.  With r = (length - thick) / 2 and h = thick / 2 the bars sit at (-h, r),
        (r, h), (h, -r), (-r, -h) with half extents (r, h), (h, r), (r, h), (h, r)."""
        length, thick = float(length), float(thick)
        if not (np.isfinite(length) and np.isfinite(thick) and 0 <= thick <= length):
            raise ValueError(f"an enclosure needs 0 <= thick <= length, got length {length}, thick {thick}")
        cx, cy = (float(c) for c in centre)
        r, h = (length - thick) / 2, thick / 2
        boxes = np.array([[cx - h, cy + r, r, h], [cx + r, cy + h, h, r], [cx + h, cy - r, r, h], [cx - r, cy - h, h, r]], np.float64)
        if solid is None:
            if kwargs:
                raise TypeError(f"enclosure: {sorted(kwargs)} need solid= (the call then returns a Walls, not the boxes)")
            return boxes
        return Walls(boxes, solid=bool(solid), **kwargs)


def wall_check(pre_xy, post_xy, boxes, radius=0.0, coef=1.0, indicator=True, counts=None):
    """The wall check of ONE step: pre_xy, post_xy [..., 2] the x, y before and after the step, boxes [M, 4] rows (cx, cy, hx, hy)
    or [..., M, 4] per position, counts [...] walls in use (None: all M) -> (cost [...] float32, clear [...] float32, wall [...]
    int64, hit [...] bool).  With a the pre-step and p the post-step position, per wall w:
        qx = |px - cx| - hx     qy = |py - cy| - hy     sdf = sqrt(max(qx, 0)^2 + max(qy, 0)^2) + min(max(qx, qy), 0)
        contact: sdf <= radius adds (radius - sdf) to the step's sum;  clear_w = sdf - radius
        mx = 0.5 (ax + px) - cx,  my likewise;  ex = 0.5 (px - ax),  ey = 0.5 (py - ay)
        hit_w = not(|mx| > hx + |ex|  or  |my| > hy + |ey|  or  |mx ey - my ex| > hx |ey| + hy |ex|)
    -- the separating-axis test of the segment a p against the closed box, without a division; with a == p it is "p in the closed
    box".  Everything is float32, every operation rounded on its own, in the device's order: four partial sums, quarter q over
    the walls q, q + 4, ..., combined as (p0 + p1) + (p2 + p3), coef applied once afterwards (indicator: cost > 0); the
    (clearance, wall) minimum over the same quarters and exchanges, the smaller clearance winning and equal clearances going to
    the smaller index (+inf and -1 without walls); hit is the OR over all walls.  sdf == radius contributes exactly 0."""
    f32 = np.float32
    a, p = np.asarray(pre_xy, f32), np.asarray(post_xy, f32)
    if a.shape != p.shape or p.shape[-1:] != (2,):
        raise ValueError(f"pre_xy and post_xy must both be [..., 2], got {a.shape} and {p.shape}")
    bx = np.asarray(boxes, f32)
    bx = bx.reshape(bx.shape[:-1] + (4,)) if bx.size else np.zeros((0, 4), f32)
    lead, M = p.shape[:-1], bx.shape[-2]
    used = np.full(lead, M) if counts is None else np.broadcast_to(np.asarray(counts), lead)
    rad, half, zero = f32(radius), f32(0.5), f32(0)
    ax, ay, px, py = a[..., 0], a[..., 1], p[..., 0], p[..., 1]
    ex, ey = half * (px - ax), half * (py - ay)
    sx, sy = half * (ax + px), half * (ay + py)
    aex, aey = np.abs(ex), np.abs(ey)
    part, clear = np.zeros((4,) + lead, f32), np.full((4,) + lead, np.inf, f32)
    wall, hit = np.full((4,) + lead, -1), np.zeros(lead, bool)
    for w in range(M):
        q = w % 4
        on = w < used
        cx, cy, hx, hy = (bx[..., w, j] for j in range(4))
        qx, qy = np.abs(px - cx) - hx, np.abs(py - cy) - hy
        ox, oy = np.maximum(qx, zero), np.maximum(qy, zero)
        sdf = np.sqrt(ox * ox + oy * oy) + np.minimum(np.maximum(qx, qy), zero)   # float32 throughout: each operation correctly rounded
        part[q] = np.where(on & (sdf <= rad), part[q] + (rad - sdf), part[q])
        cl = sdf - rad
        closer = on & (cl < clear[q])                                             # ascending w: equal clearances keep the lower index
        clear[q], wall[q] = np.where(closer, cl, clear[q]), np.where(closer, w, wall[q])
        mx, my = sx - cx, sy - cy
        apart = (np.abs(mx) > hx + aex) | (np.abs(my) > hy + aey) | (np.abs(mx * ey - my * ex) > hx * aey + hy * aex)
        hit = hit | (on & ~apart)

    def closer_of(u, v):
        (cu, wu), (cv, wv) = u, v
        take = (cv < cu) | ((cv == cu) & (wv < wu))
        return np.where(take, cv, cu), np.where(take, wv, wu)
    total = f32(coef) * ((part[0] + part[1]) + (part[2] + part[3]))
    cl, wi = closer_of(closer_of((clear[0], wall[0]), (clear[1], wall[1])), closer_of((clear[2], wall[2]), (clear[3], wall[3])))
    if indicator:
        total = (total > 0).astype(f32)
    return np.asarray(total, f32), np.asarray(cl, f32), np.asarray(wi, np.int64), np.asarray(hit, bool)


def wall_fold(record, pre_xy, post_xy, stepped, walls, step0=0):
    """The carried wall record after the steps step0 .. step0 + T - 1: record [n][7] float64 (sum of step costs, contact steps
    (cost > 0), the first such step as a global 1-based number or -1, the minimum clearance over the run -- NaN before the
    robot's first step, +inf without walls --, the wall's index at that minimum, first attainment kept, or -1, crossing steps,
    the first crossing step or -1), pre_xy / post_xy [T][n][2] the positions before and after each step, stepped [T][n], walls
    a Walls.  Returns a new [n][7]; a robot accounts only for the steps in which it stepped."""
    rec = np.array(record, np.float64)
    pre, post = np.asarray(pre_xy, np.float32), np.asarray(post_xy, np.float32)
    stepped = np.asarray(stepped, bool)
    T, n = stepped.shape
    walls.check_robots(n)
    if rec.shape != (n, 7) or pre.shape != (T, n, 2) or post.shape != (T, n, 2):
        raise ValueError(f"record must be [{n}][7] and pre_xy, post_xy [{T}][{n}][2], got {rec.shape}, {pre.shape} and {post.shape}")
    sc = np.zeros(n, np.int64) if walls.scene is None else walls.scene.astype(np.int64)
    boxes, counts = walls.table[sc], walls.counts[sc]                             # [n, M, 4], [n]
    for t in range(T):
        s = stepped[t]
        cost, clear, wall, hit = wall_check(pre[t], post[t], boxes, walls.radius, walls.cost, walls.indicator, counts)
        cost, clear = cost.astype(np.float64), clear.astype(np.float64)
        rec[:, 0] += np.where(s, cost, 0.0)                                       # float64, one step after the other
        touch = s & (cost > 0)
        rec[:, 1] += touch
        rec[:, 2] = np.where(touch & (rec[:, 2] < 0), step0 + t + 1, rec[:, 2])
        best = np.where(np.isnan(rec[:, 3]), np.inf, rec[:, 3])
        closer = s & (clear < best)
        rec[:, 3] = np.where(s, np.where(closer, clear, best), rec[:, 3])
        rec[:, 4] = np.where(closer, wall, rec[:, 4])
        cross = s & hit
        rec[:, 5] += cross
        rec[:, 6] = np.where(cross & (rec[:, 6] < 0), step0 + t + 1, rec[:, 6])
    return rec


# ---- solid walls (Walls(..., solid=True)): the step's proposed position is resolved against the boxes inside the environment
# step, between the dynamics and the goal test.  Stated here once; the device (csrc/kernels_wall.h: wall_resolve) is held to it
# bit for bit, the host loop applies it as it stands.
BLOCKED_START = (0, -1, 0, 0)   # a robot's blocked record before its first step: blocked steps, first blocked step, stopped, inside


def goal_propose32(pos, vel, act, mix, dt, extent, P):
    """The device's velocity and position update (csrc/kernels_env.h: goal_advance) bit for bit: pos, vel [..., >= P] float32,
    act [..., A], mix [3][>= A] -> (proposed pos [..., P], vel [..., P]) float32.  cmd_j accumulates mix[j][k] act[k] in k order
    by fused multiply-adds from 0; vel_j = fma(0.8, vel_j, 0.2 cmd_j); pos_j = clamp(fma(dt, vel_j, pos_j), -extent, extent)."""
    f32 = np.float32
    pos, vel, act, mix = (np.asarray(x, f32) for x in (pos, vel, act, mix))
    lead = np.broadcast_shapes(pos.shape[:-1], vel.shape[:-1], act.shape[:-1])
    new_pos, new_vel = [], []
    for j in range(int(P)):
        cmd = np.zeros(lead, f32)
        for k in range(act.shape[-1]):
            cmd = _fma32(mix[j, k], act[..., k], cmd).reshape(lead)
        v = _fma32(f32(0.8), vel[..., j], f32(0.2) * cmd).reshape(lead)
        p = np.minimum(np.maximum(_fma32(f32(dt), v, pos[..., j]).reshape(lead), -f32(extent)), f32(extent))
        new_vel.append(v)
        new_pos.append(p.astype(f32))
    return np.stack(new_pos, -1), np.stack(new_vel, -1)


def wall_block(a_xy, p_xy, boxes, radius=0.0, counts=None):
    """Solid walls, ONE step: a_xy [..., 2] the x, y before the step, p_xy [..., 2] the x, y the dynamics propose (after the clamp
    to the extent), boxes [M, 4] or [..., M, 4] rows (cx, cy, hx, hy), counts [...] walls in use (None: all M) -> (q_xy [..., 2]
    float32 the position the step ends on, code [...] int64, inside [...] bool).  Float32, every operation rounded on its own.
        Hx = hx + radius,  Hy = hy + radius                       (the robot's centre against the closed square-inflated box)
        a wall with |ax - cx| <= Hx and |ay - cy| <= Hy does not hold in this step (inside: any such wall) -- a robot that
        starts within an inflated box can leave it;
        seg_hit(a, c): the OR over the other walls of wall_check's separating test of the segment a c with Hx, Hy for hx, hy;
        candidates in order: c0 = (px, py), c1 = (px, ay), c2 = (ax, py), c3 = (ax, ay); the first one without a hit is taken,
        c3 untested; code = its number.
    A dropped axis (y for 1, x for 2, both for 3) has its velocity component set to +0.0 by the caller (wall_block_velocity).
    Float add and the non-negative products are monotone, so a segment that meets a closed un-inflated box meets its inflated
    one: with inside False, wall_check(a, q) reports no crossing."""
    f32 = np.float32
    a, p = np.asarray(a_xy, f32), np.asarray(p_xy, f32)
    if a.shape != p.shape or p.shape[-1:] != (2,):
        raise ValueError(f"a_xy and p_xy must both be [..., 2], got {a.shape} and {p.shape}")
    bx = np.asarray(boxes, f32)
    bx = bx.reshape(bx.shape[:-1] + (4,)) if bx.size else np.zeros((0, 4), f32)
    lead, M = p.shape[:-1], bx.shape[-2]
    used = np.full(lead, M) if counts is None else np.broadcast_to(np.asarray(counts), lead)
    rad, half = f32(radius), f32(0.5)
    ax, ay, px, py = a[..., 0], a[..., 1], p[..., 0], p[..., 1]
    walls = []
    inside = np.zeros(lead, bool)
    for w in range(M):
        cx, cy = bx[..., w, 0], bx[..., w, 1]
        Hx, Hy = bx[..., w, 2] + rad, bx[..., w, 3] + rad
        on = w < used
        within = on & (np.abs(ax - cx) <= Hx) & (np.abs(ay - cy) <= Hy)
        inside = inside | within
        walls.append((cx, cy, Hx, Hy, on & ~within))

    def seg_hit(qx, qy):
        ex, ey = half * (qx - ax), half * (qy - ay)
        sx, sy = half * (ax + qx), half * (ay + qy)
        aex, aey = np.abs(ex), np.abs(ey)
        hit = np.zeros(lead, bool)
        for cx, cy, Hx, Hy, holds in walls:
            mx, my = sx - cx, sy - cy
            apart = (np.abs(mx) > Hx + aex) | (np.abs(my) > Hy + aey) | (np.abs(mx * ey - my * ex) > Hx * aey + Hy * aex)
            hit = hit | (holds & ~apart)
        return hit
    h0, h1, h2 = seg_hit(px, py), seg_hit(px, ay), seg_hit(ax, py)
    code = np.where(~h0, 0, np.where(~h1, 1, np.where(~h2, 2, 3)))
    qx = np.where((code == 0) | (code == 1), px, ax)
    qy = np.where((code == 0) | (code == 2), py, ay)
    return np.stack([qx, qy], -1).astype(f32), np.asarray(code, np.int64), inside


def wall_block_velocity(vel, code):
    """vel [..., P] after the step's velocity update -> the velocity the step ends with: the component of every dropped axis
    (y for code 1, x for 2, both for 3) is +0.0; z is untouched."""
    v = np.array(vel, copy=True)
    code = np.asarray(code)
    v[..., 0] = np.where((code == 2) | (code == 3), v.dtype.type(0), v[..., 0])
    v[..., 1] = np.where((code == 1) | (code == 3), v.dtype.type(0), v[..., 1])
    return v


def wall_blocked_fold(record, code, inside, stepped, step0=0):
    """The carried blocked record after the steps step0 .. step0 + T - 1: record [n][4] integers (blocked steps: code != 0, the
    first such step as a global 1-based number or -1, fully stopped steps: code 3, steps in which a wall did not hold: inside),
    code / inside / stepped [T][n].  Returns a new [n][4] int64; a robot accounts only for the steps in which it stepped."""
    rec = np.array(record, np.int64)
    code, inside, stepped = np.asarray(code), np.asarray(inside, bool), np.asarray(stepped, bool)
    T, n = stepped.shape
    if rec.shape != (n, 4) or code.shape != (T, n) or inside.shape != (T, n):
        raise ValueError(f"record must be [{n}][4] and code, inside [{T}][{n}], got {rec.shape}, {code.shape} and {inside.shape}")
    for t in range(T):
        blocked = stepped[t] & (code[t] != 0)
        rec[:, 0] += blocked
        rec[:, 1] = np.where(blocked & (rec[:, 1] < 0), step0 + t + 1, rec[:, 1])
        rec[:, 2] += stepped[t] & (code[t] == 3)
        rec[:, 3] += stepped[t] & inside[t]
    return rec


# ---- solid teams (Teams(..., solid=True)): team-mates are obstacles inside the environment step.  A mate is one more box of
# wall_block's rule, one that moves: the closed square of half-width `separation` around where the mate stands.  Stated here once;
# the device (csrc/kernels_team_solid.h: team_resolve) is held to it bit for bit.
TEAM_BLOCKED_START = (0, -1, 0, 0)   # a robot's team-blocked record before its first step: steps blocked by a mate, first, stopped, inside


def team_block(a_xy, p_xy, mates_xy, sep, boxes=None, radius=0.0, counts=None):
    """Solid teams, ONE robot's resolve: a_xy [..., 2] the x, y before the step, p_xy [..., 2] the x, y the dynamics propose,
    mates_xy [..., J, 2] where each of its J mates stands (team_block_step says which position that is), sep the separation;
    with solid walls also boxes [M, 4] or [..., M, 4], radius and counts as wall_block takes them -> (q_xy [..., 2] float32,
    code [...] int64, inside [...] bool, by_mate [...] bool, by_wall [...] bool, wall_inside [...] bool).
    It is wall_block's rule over one list of inflated boxes, float32, every operation rounded on its own:
        mate j:  centre c_j, Hx = Hy = sep exactly (no addition)          wall w:  Hx = hx + radius, Hy = hy + radius
        a box with |ax - cx| <= Hx and |ay - cy| <= Hy does not hold in this step -- `inside`: any such mate, `wall_inside`: any
        such wall -- so mates that start too close can separate;
        candidates c0 = (px, py), c1 = (px, ay), c2 = (ax, py), c3 = (ax, ay) in wall_block's order with its three-axis segment
        test against every box that holds, mates and walls at once; the first candidate without a hit is taken, c3 untested.
    The split of a blocked step between the two records: by_mate -- a rejected candidate (c0 .. c(code - 1)) met a mate's square;
    by_wall -- a rejected candidate met a wall.  Both can hold in one step; with code 0 neither does.  A step blocked by walls
    only has by_mate False and is counted in the walls' blocked record alone (team_block_fold).
    With boxes None the first three results are wall_block(a, p, [(cx, cy, sep, sep) per mate], radius=0.0) bit for bit."""
    f32 = np.float32
    a, p = np.asarray(a_xy, f32), np.asarray(p_xy, f32)
    if a.shape != p.shape or p.shape[-1:] != (2,):
        raise ValueError(f"a_xy and p_xy must both be [..., 2], got {a.shape} and {p.shape}")
    lead = p.shape[:-1]
    mt = np.asarray(mates_xy, f32)
    mt = mt.reshape(mt.shape[:-1] + (2,)) if mt.size else np.zeros(lead + (0, 2), f32)
    if mt.shape[:-2] != lead:
        raise ValueError(f"mates_xy must be {lead + ('J', 2)}, got {mt.shape}")
    s, half = f32(sep), f32(0.5)
    ax, ay, px, py = a[..., 0], a[..., 1], p[..., 0], p[..., 1]
    held = []                                                     # (cx, cy, Hx, Hy, holds, mate)
    inside, wall_inside = np.zeros(lead, bool), np.zeros(lead, bool)
    for j in range(mt.shape[-2]):
        cx, cy = mt[..., j, 0], mt[..., j, 1]
        within = (np.abs(ax - cx) <= s) & (np.abs(ay - cy) <= s)
        inside = inside | within
        held.append((cx, cy, s, s, ~within, True))
    if boxes is not None:
        bx = np.asarray(boxes, f32)
        bx = bx.reshape(bx.shape[:-1] + (4,)) if bx.size else np.zeros((0, 4), f32)
        M, rad = bx.shape[-2], f32(radius)
        used = np.full(lead, M) if counts is None else np.broadcast_to(np.asarray(counts), lead)
        for w in range(M):
            cx, cy = bx[..., w, 0], bx[..., w, 1]
            Hx, Hy = bx[..., w, 2] + rad, bx[..., w, 3] + rad
            on = w < used
            within = on & (np.abs(ax - cx) <= Hx) & (np.abs(ay - cy) <= Hy)
            wall_inside = wall_inside | within
            held.append((cx, cy, Hx, Hy, on & ~within, False))

    def seg_hit(qx, qy):
        ex, ey = half * (qx - ax), half * (qy - ay)
        sx, sy = half * (ax + qx), half * (ay + qy)
        aex, aey = np.abs(ex), np.abs(ey)
        hit = [np.zeros(lead, bool), np.zeros(lead, bool)]        # walls, mates
        for cx, cy, Hx, Hy, holds, mate in held:
            mx, my = sx - cx, sy - cy
            apart = (np.abs(mx) > Hx + aex) | (np.abs(my) > Hy + aey) | (np.abs(mx * ey - my * ex) > Hx * aey + Hy * aex)
            hit[mate] = hit[mate] | (holds & ~apart)
        return hit
    (w0, m0), (w1, m1), (w2, m2) = seg_hit(px, py), seg_hit(px, ay), seg_hit(ax, py)
    h0, h1, h2 = w0 | m0, w1 | m1, w2 | m2
    code = np.where(~h0, 0, np.where(~h1, 1, np.where(~h2, 2, 3)))
    by_mate = ((code >= 1) & m0) | ((code >= 2) & m1) | ((code >= 3) & m2)
    by_wall = ((code >= 1) & w0) | ((code >= 2) & w1) | ((code >= 3) & w2)
    qx = np.where((code == 0) | (code == 1), px, ax)
    qy = np.where((code == 0) | (code == 2), py, ay)
    return np.stack([qx, qy], -1).astype(f32), np.asarray(code, np.int64), inside, by_mate, by_wall, wall_inside


def team_block_scalar(a, p, mates, sep):
    """team_block without walls for ONE robot, restated with Python loops over np.float32 scalars: a, p (x, y), mates a list of
    (x, y) -> ((qx, qy), code, inside, by_mate).  The array form is held to it by the tests."""
    f32 = np.float32
    ax, ay, px, py, s, half = f32(a[0]), f32(a[1]), f32(p[0]), f32(p[1]), f32(sep), f32(0.5)
    boxes = [(f32(cx), f32(cy)) for cx, cy in mates]
    within = [bool(abs(ax - cx) <= s and abs(ay - cy) <= s) for cx, cy in boxes]
    by_mate = False
    for code, (qx, qy) in enumerate(((px, py), (px, ay), (ax, py))):
        ex, ey = half * (qx - ax), half * (qy - ay)
        sx, sy = half * (ax + qx), half * (ay + qy)
        aex, aey = abs(ex), abs(ey)
        hit = False
        for (cx, cy), inside in zip(boxes, within):
            mx, my = sx - cx, sy - cy
            apart = abs(mx) > s + aex or abs(my) > s + aey or abs(f32(mx * ey) - f32(my * ex)) > f32(s * aey) + f32(s * aex)
            hit = hit or (not inside and not apart)
        if not hit:
            return (qx, qy), code, any(within), by_mate
        by_mate = True
    return (ax, ay), 3, any(within), True


def team_block_step(stand_xy, prop_xy, stepped, teams, walls=None):
    """Solid teams, ONE global step of all n robots: stand_xy [n][2] where every robot stands before the step (for a robot that
    steps: its pre-step x, y), prop_xy [n][2] the x, y the dynamics propose for the robots that step (ignored for the others),
    stepped [n], teams a Teams, walls a solid Walls or None -> (q_xy [n][2] where every robot stands after the step, code,
    inside, by_mate, by_wall, wall_inside [n]; zeros / False for a robot that did not step).
    The order is serial inside a team, by team-local index m = 0 .. size - 1: member m resolves (team_block) against the mates
    with a lower index where they stand AFTER their resolve of this step, against the mates with a higher index where they stood
    BEFORE the step; a mate that does not step (finished, not released, inactive in this call) counts where it stands.  Teams
    are independent of each other."""
    f32 = np.float32
    pos = np.array(stand_xy, f32)
    prop, stepped = np.asarray(prop_xy, f32), np.asarray(stepped, bool)
    n = stepped.shape[0]
    teams.check_robots(n)
    if pos.shape != (n, 2) or prop.shape != (n, 2):
        raise ValueError(f"stand_xy and prop_xy must be [{n}][2], got {pos.shape} and {prop.shape}")
    G = teams.size
    code, flags = np.zeros(n, np.int64), np.zeros((4, n), bool)
    boxes = counts = None
    if walls is not None:
        walls.check_robots(n)
        sc = np.zeros(n, np.int64) if walls.scene is None else walls.scene.astype(np.int64)
        boxes, counts = walls.table[sc], walls.counts[sc]
    for m in range(G):
        idx = np.arange(m, n, G)
        mates = pos.reshape(n // G, G, 2)[:, [j for j in range(G) if j != m]]
        q, c, *fl = team_block(pos[idx], prop[idx], mates, teams.separation, None if boxes is None else boxes[idx],
                               0.0 if walls is None else walls.radius, None if counts is None else counts[idx])
        s = stepped[idx]
        pos[idx] = np.where(s[:, None], q, pos[idx])
        code[idx] = np.where(s, c, 0)
        for k in range(4):
            flags[k, idx] = s & fl[k]
    return (pos, code) + tuple(flags)


def team_block_fold(record, code, inside, by_mate, stepped, step0=0):
    """The carried team-blocked record after the steps step0 .. step0 + T - 1: record [n][4] integers (steps blocked by a mate:
    by_mate, the first such step as a global 1-based number or -1, such steps with no move at all: code 3, steps inside a mate's
    square), code / inside / by_mate / stepped [T][n].  It is wall_blocked_fold on the code of the steps a mate blocked; with
    solid walls the walls' own record is wall_blocked_fold(record, where(by_wall, code, 0), wall_inside, stepped, step0)."""
    return wall_blocked_fold(record, np.where(np.asarray(by_mate, bool), np.asarray(code), 0), inside, stepped, step0)


# ---- grid planner: walls and hazards to waypoints.  This project's own rule; it is stated here once and the device
# (csrc/kernels_plan.h) is held to it bit for bit.  x and y only, as for hazards and walls.
PLAN_CELLS = (32, 64, 128)
PLAN_STEP, PLAN_DIAG = 5, 7          # integer chamfer costs of an orthogonal and of a diagonal move
PLAN_DIRS = ((1, 0), (0, 1), (-1, 0), (0, -1), (1, 1), (-1, 1), (-1, -1), (1, -1))   # E, N, W, S, NE, NW, SW, SE: (dx, dy)
PLANNED, UNREACHABLE, TRUNCATED, UNCONVERGED = 0, 1, 2, 3   # status of a robot's plan (3: a loop bound was hit; the rule never returns it)


class GridSpec:
    """A square grid of `cells` x `cells` (G in PLAN_CELLS) over [-extent, extent]^2 and the clearance `inflate` a blocked cell's
    centre keeps from walls and hazards (None: the walls' robot radius + one cell, filled in by grid_occupancy).  The float32
    numbers every path uses: extent, h = 2 extent / G, inv_h = G / (2 extent) (each computed in float64 and rounded once) and
    inflate.  Checked on construction (ValueError).  Cell (ix, iy) has the flat index iy * G + ix."""

    def __init__(self, extent, cells=64, inflate=None):
        if isinstance(cells, bool) or not isinstance(cells, (int, np.integer)) or int(cells) not in PLAN_CELLS:
            raise ValueError(f"grid cells must be one of {PLAN_CELLS}, got {cells!r}")
        extent = float(extent)
        if not np.isfinite(extent) or extent <= 0:
            raise ValueError(f"grid extent must be finite and > 0, got {extent}")
        self.cells = int(cells)
        self.extent = np.float32(extent)
        self.h, self.inv_h = np.float32(2.0 * float(self.extent) / self.cells), np.float32(self.cells / (2.0 * float(self.extent)))
        if not (np.isfinite(self.h) and self.h > 0 and np.isfinite(self.inv_h) and self.inv_h > 0):
            raise ValueError(f"grid extent {extent} does not give a finite cell size in float32")
        self.inflate = None
        if inflate is not None:
            inflate = float(inflate)
            if not np.isfinite(inflate) or inflate < 0:
                raise ValueError(f"grid inflate must be finite and >= 0, got {inflate}")
            self.inflate = np.float32(inflate)

    def inflate_for(self, walls=None):
        """the float32 inflate in force: the given one, else the walls' radius (0 without walls) + h, rounded once"""
        if self.inflate is not None:
            return self.inflate
        return np.float32(np.float32(0.0 if walls is None else walls.radius) + self.h)

    def cell_of(self, xy):
        """[..., 2] -> (ix, iy) int64: clamp(floor((x + extent) * inv_h), 0, G - 1), float32, add and multiply rounded on their own"""
        p = np.asarray(xy, np.float32)
        c = np.floor((p + self.extent) * self.inv_h)
        c = np.clip(c, 0, self.cells - 1).astype(np.int64)
        return c[..., 0], c[..., 1]

    def centre(self, i):
        """cell coordinate(s) -> float32 centre coordinate: -extent + (i + 0.5) * h, each operation rounded"""
        return (-self.extent) + (np.asarray(i).astype(np.float32) + np.float32(0.5)) * self.h


def plan_scene(walls=None, hazards=None):
    """-> (S, scene [n] int32 or None) of a planning scene: walls and hazards must agree on the number of scenes and on the scene
    index per robot (ValueError); neither: one empty scene."""
    if walls is not None and not isinstance(walls, Walls):
        raise TypeError(f"walls must be a mobrob_amd.envs.goal_rules.Walls, not {type(walls).__name__}")
    if hazards is not None and not isinstance(hazards, Hazards):
        raise TypeError(f"hazards must be a mobrob_amd.envs.goal_rules.Hazards (moving hazards are not planned around), not {type(hazards).__name__}")
    return _scene_agreement(walls, hazards)


def _scene_agreement(walls, hazards):
    """plan_scene's checks and result for walls and hazards (static or moving) whose types are settled"""
    if walls is not None and hazards is not None:
        if walls.n_scenes != hazards.n_scenes:
            raise ValueError(f"plan: walls have {walls.n_scenes} scenes, hazards {hazards.n_scenes}")
        if (walls.scene is None) != (hazards.scene is None) or (walls.scene is not None and not np.array_equal(walls.scene, hazards.scene)):
            raise ValueError("plan: walls and hazards must agree on the scene index per robot")
    src = walls if walls is not None else hazards
    return (1, None) if src is None else (src.n_scenes, src.scene)


def grid_occupancy(spec, walls=None, hazards=None):
    """bool [S][G][G] (scene, iy, ix): a cell is blocked if its centre p has sdf <= inflate to a wall of the scene (wall_check's sdf,
    in its float32 arithmetic) or d <= radius_k + inflate to a hazard k of the scene (d = sqrt(dx^2 + dy^2) as team_cost computes
    a distance; the sum radius_k + inflate rounded once).  Equality blocks.  inflate: spec.inflate_for(walls)."""
    f32 = np.float32
    S, _ = plan_scene(walls, hazards)
    G, zero = spec.cells, f32(0)
    inflate = spec.inflate_for(walls)
    c = spec.centre(np.arange(G))
    px, py = np.broadcast_to(c[None, :], (G, G)), np.broadcast_to(c[:, None], (G, G))
    occ = np.zeros((S, G, G), bool)
    for s in range(S):
        for w in range(0 if walls is None else int(walls.counts[s])):
            cx, cy, hx, hy = (f32(v) for v in walls.table[s, w])
            qx, qy = np.abs(px - cx) - hx, np.abs(py - cy) - hy
            ox, oy = np.maximum(qx, zero), np.maximum(qy, zero)
            sdf = np.sqrt(ox * ox + oy * oy) + np.minimum(np.maximum(qx, qy), zero)
            occ[s] |= sdf <= inflate
        if hazards is not None:
            occ[s] |= _hazard_rows_block(px, py, hazards.table[s, :int(hazards.counts[s])], inflate)
    return occ


def _hazard_rows_block(px, py, rows, inflate):
    """grid_occupancy's hazard test of the centres (px, py) against the float32 rows [m][3]: bool, True where a row blocks"""
    f32 = np.float32
    out = np.zeros(px.shape, bool)
    for row in rows:
        x, y, r = (f32(v) for v in row)
        dx, dy = px - x, py - y
        out |= np.sqrt(dx * dx + dy * dy) <= f32(r + inflate)
    return out


def plan_move_ok(occ, ix, iy, k):
    """May a robot in the free cell (ix, iy) of occ [G][G] make move k of PLAN_DIRS?  The target lies in the grid and is free; a
    diagonal also needs both orthogonal cells that share the corner free (no corner cutting).  Symmetric in the two cells."""
    G = occ.shape[0]
    dx, dy = PLAN_DIRS[k]
    jx, jy = ix + dx, iy + dy
    if not (0 <= jx < G and 0 <= jy < G) or occ[jy, jx]:
        return False
    return k < 4 or not (occ[iy, jx] or occ[jy, ix])


def grid_field(occ_scene, goal_cell):
    """int32 [G][G]: the cost-to-go of every cell to the cell with flat index goal_cell over eight-connected moves (PLAN_STEP
    orthogonal, PLAN_DIAG diagonal, plan_move_ok); -1 for blocked and unreachable cells, all -1 for a blocked goal cell.  Dijkstra;
    the field is the unique fixed point of d[c] = min(d[nb] + w) with d[goal] = 0, so any relaxation order gives the same."""
    import heapq
    occ = np.asarray(occ_scene, bool)
    G = occ.shape[0]
    d = np.full((G, G), -1, np.int32)
    gx, gy = int(goal_cell) % G, int(goal_cell) // G
    if not 0 <= int(goal_cell) < G * G:
        raise ValueError(f"goal cell must lie in 0 .. {G * G - 1}, got {goal_cell}")
    if occ[gy, gx]:
        return d
    d[gy, gx] = 0
    heap = [(0, gy, gx)]
    while heap:
        dc, iy, ix = heapq.heappop(heap)
        if dc != d[iy, ix]:
            continue
        for k, (dx, dy) in enumerate(PLAN_DIRS):
            if plan_move_ok(occ, ix, iy, k):
                nd = dc + (PLAN_STEP if k < 4 else PLAN_DIAG)
                if d[iy + dy, ix + dx] < 0 or nd < d[iy + dy, ix + dx]:
                    d[iy + dy, ix + dx] = nd
                    heapq.heappush(heap, (nd, iy + dy, ix + dx))
    return d


def grid_walk(field, occ_scene, spec, start_xy, goal_xy):
    """The cells of grid_path's walk -> (cells [(ix, iy), ...] from the start's cell to the goal's, directions taken, status):
    status UNREACHABLE (empty lists) if the start cell or the goal cell is blocked or field[start] < 0."""
    sx, sy = (int(v) for v in spec.cell_of(np.asarray(start_xy, np.float32)[:2]))
    gx, gy = (int(v) for v in spec.cell_of(np.asarray(goal_xy, np.float32)[:2]))
    return grid_walk_cells(field, occ_scene, (sx, sy), (gx, gy))


def grid_walk_cells(field, occ_scene, start_cell, goal_cell):
    """grid_walk between two cells (ix, iy): the descent rule itself, stated here once (grid_walk, and every leg of spec_plan)"""
    occ, d = np.asarray(occ_scene, bool), np.asarray(field)
    G = occ.shape[0]
    (sx, sy), (gx, gy) = start_cell, goal_cell
    if occ[sy, sx] or occ[gy, gx] or d[sy, sx] < 0:
        return [], [], UNREACHABLE
    cells, dirs, prev = [(sx, sy)], [], -1
    ix, iy = sx, sy
    while (ix, iy) != (gx, gy):
        def descends(k):
            return plan_move_ok(occ, ix, iy, k) and d[iy + PLAN_DIRS[k][1], ix + PLAN_DIRS[k][0]] >= 0 and \
                d[iy + PLAN_DIRS[k][1], ix + PLAN_DIRS[k][0]] + (PLAN_STEP if k < 4 else PLAN_DIAG) == d[iy, ix]
        k = prev if prev >= 0 and descends(prev) else next((j for j in range(8) if descends(j)), -1)
        if k < 0 or len(cells) > G * G:
            raise ValueError("grid_path: the field is not the cost-to-go of this occupancy and goal")
        ix, iy, prev = ix + PLAN_DIRS[k][0], iy + PLAN_DIRS[k][1], k
        cells.append((ix, iy))
        dirs.append(k)
    return cells, dirs, PLANNED


def grid_path(field, occ_scene, spec, start_xy, goal_xy, K, walk=None):
    """One robot's waypoints -> (waypoints [K][2] float32, count, status, cost).  The walk starts in the start's cell and steps to
    a neighbour nb with field[nb] + w == field[c] under plan_move_ok: the previous direction if it qualifies, else the lowest index
    of PLAN_DIRS.  A cell's centre is a waypoint when the direction leaving it differs from the direction entering it (the start
    cell emits nothing); the last waypoint is goal_xy itself.  count: the waypoints of the full path; the first min(count, K)
    are written, the other slots are zero.  status PLANNED, UNREACHABLE (start or goal cell blocked, or no path: count 0, cost
    -1) or TRUNCATED (count > K).  cost = field[start cell].  A start in the goal's cell gives the single waypoint goal_xy.
    walk: the (cells, directions, status) to take the waypoints from, None: grid_walk's."""
    K = int(K)
    if K < 1:
        raise ValueError("max_waypoints must be >= 1")
    wp = np.zeros((K, 2), np.float32)
    cells, dirs, status = grid_walk(field, occ_scene, spec, start_xy, goal_xy) if walk is None else walk
    if status == UNREACHABLE:
        return wp, 0, UNREACHABLE, -1
    count = 0
    for j in range(1, len(cells) - 1):
        if dirs[j] != dirs[j - 1]:
            if count < K:
                wp[count] = spec.centre(cells[j][0]), spec.centre(cells[j][1])
            count += 1
    if count < K:
        wp[count] = np.asarray(goal_xy, np.float32)[:2]
    count += 1
    sx, sy = cells[0]
    return wp, count, TRUNCATED if count > K else PLANNED, int(np.asarray(field)[sy, sx])


def plan_fields(spec, occupancy, scene, goal):
    """Robots sharing a scene and a goal cell share a field -> (field_of [n] int32, field_goal_cell [F] int32, field_scene [F]
    int32), fields numbered in ascending (scene, goal cell).  scene [n] or None (scene 0), goal [n][>= 2]."""
    goal = np.asarray(goal, np.float32)
    n, G = goal.shape[0], spec.cells
    gx, gy = spec.cell_of(goal[:, :2])
    sc = np.zeros(n, np.int64) if scene is None else np.asarray(scene, np.int64)
    key = sc * (G * G) + gy * G + gx
    uniq, inv = np.unique(key, return_inverse=True)
    return inv.reshape(n).astype(np.int32), (uniq % (G * G)).astype(np.int32), (uniq // (G * G)).astype(np.int32)


def grid_dilate(occ_scene):
    """bool [G][G]: a cell is True when a cell of its 3 x 3 neighbourhood that lies in the grid is blocked (cells outside the grid
    count as free): the cells that are not "clear" at margin 1."""
    occ = np.asarray(occ_scene, bool)
    G = occ.shape[0]
    pad = np.zeros((G + 2, G + 2), bool)
    pad[1:-1, 1:-1] = occ
    out = np.zeros((G, G), bool)
    for dy in range(3):
        for dx in range(3):
            out |= pad[dy:dy + G, dx:dx + G]
    return out


def los_blocked(occ_scene, margin):
    """The map grid_los tests a cell against: the occupancy itself at margin 0, grid_dilate of it at margin 1."""
    if isinstance(margin, bool) or margin not in (0, 1):
        raise ValueError(f"line-of-sight margin must be 0 or 1, got {margin!r}")
    return np.asarray(occ_scene, bool) if margin == 0 else grid_dilate(occ_scene)


def los_walk(blk, a, b):
    """grid_los on the map `blk` of cells that are not clear -> (visible, steps taken, corners met)."""
    (x, y), (x1, y1) = (int(a[0]), int(a[1])), (int(b[0]), int(b[1]))
    dx, dy = abs(x1 - x), abs(y1 - y)
    sx, sy = (1 if x1 > x else -1), (1 if y1 > y else -1)
    ix = iy = steps = corners = 0
    if blk[y, x]:
        return False, 0, 0
    while ix < dx or iy < dy:
        t = (1 + 2 * ix) * dy - (1 + 2 * iy) * dx
        steps += 1
        if t < 0:
            x, ix = x + sx, ix + 1
        elif t > 0:
            y, iy = y + sy, iy + 1
        else:                                   # exactly through a cell corner: no corner cutting, as plan_move_ok
            corners += 1
            if blk[y, x + sx] or blk[y + sy, x]:
                return False, steps, corners
            x, y, ix, iy = x + sx, y + sy, ix + 1, iy + 1
        if blk[y, x]:
            return False, steps, corners
    return True, steps, corners


def grid_los(occ, a, b, margin=0):
    """Is cell b = (x1, y1) visible from cell a = (x0, y0) on occ [G][G]?  Integers only: the supercover of the segment between the
    two centres.  With dx = |x1 - x0|, dy = |y1 - y0|, signs sx, sy and counters ix = iy = 0: false if a is not clear; while ix < dx
    or iy < dy, t = (1 + 2 ix) dy - (1 + 2 iy) dx; t < 0 steps in x, t > 0 steps in y, t == 0 (the segment passes exactly through a
    cell corner) needs both cells that share the corner, (x + sx, y) and (x, y + sy), clear and then steps in both; false if the
    cell stepped into is not clear.  At most dx + dy steps; symmetric in a and b.  A cell is clear at margin 0 when it is not
    blocked, at margin 1 when no in-grid cell of its 3 x 3 neighbourhood is blocked."""
    return los_walk(los_blocked(occ, margin), a, b)[0]


def grid_smooth(cells, occ, margin=1, blocked=None):
    """Line-of-sight smoothing of grid_walk's cells c_0 .. c_L -> the ascending indices of the cells kept as waypoints.  Anchor
    i = 0, j = 1; while j < L: if grid_los(occ, c_i, c_{j+1}, margin) then j += 1, else emit j, i = j, j += 1.  Adjacent cells are
    never tested (they are a move of the walk), so every margin makes progress.  blocked: los_blocked(occ, margin), computed
    once by a caller with many walks."""
    blk = los_blocked(occ, margin) if blocked is None else blocked
    L, out, i, j = len(cells) - 1, [], 0, 1
    while j < L:
        if not los_walk(blk, cells[i], cells[j + 1])[0]:
            out.append(j)
            i = j
        j += 1
    return out


def grid_path_smooth(field, occ_scene, spec, start_xy, goal_xy, K, margin=1, blocked=None, walk=None):
    """grid_path with line-of-sight smoothing -> (waypoints [K][2] float32, count, status, cost, moves): the waypoints are the
    centres of the cells grid_smooth keeps of the walk, then goal_xy itself; count, status, cost and the zeroed slots mean what
    they mean in grid_path; moves = L, the moves of the walk (0 where none was made).  walk: as grid_path's."""
    K = int(K)
    if K < 1:
        raise ValueError("max_waypoints must be >= 1")
    wp = np.zeros((K, 2), np.float32)
    cells, _, status = grid_walk(field, occ_scene, spec, start_xy, goal_xy) if walk is None else walk
    if status == UNREACHABLE:
        return wp, 0, UNREACHABLE, -1, 0
    keep = grid_smooth(cells, occ_scene, margin, blocked)
    for count, j in enumerate(keep[:K]):
        wp[count] = spec.centre(cells[j][0]), spec.centre(cells[j][1])
    count = len(keep)
    if count < K:
        wp[count] = np.asarray(goal_xy, np.float32)[:2]
    count += 1
    sx, sy = cells[0]
    return wp, count, TRUNCATED if count > K else PLANNED, int(np.asarray(field)[sy, sx]), len(cells) - 1


def grid_plan(spec, walls, hazards, start, goal, K, occupancy=None, fields=None, smooth=False, margin=1, clearance=None):
    """The whole plan of n robots by the rule: start, goal [n][P] (P = 2 or 3) -> dict of waypoints [n][K][P] float32 (z of every
    waypoint: the goal's), n_waypoints, count, status, cost [n] int32, occupancy bool [S][G][G], fields int32 [F][G][G], field_of,
    field_goal_cell, field_scene.  `occupancy` / `fields`: a previous call's, reused (the same scene and goals).  smooth: the
    paths by grid_path_smooth with the line-of-sight `margin` (0 or 1), and `moves` [n] int32 beside them.
    clearance: None, or (reach, weight): the clearance-aware plan (grid_surcharge, grid_field_cost, grid_walk_cost below) --
    `fields` are then cost fields with the surcharges in them (reuse only such a call's), `cost` includes the surcharges paid, and
    the dict gains surcharge uint8 [S][G][G] and clearance_min [n] int32 (grid_walk_clearance)."""
    start, goal = np.asarray(start, np.float32), np.asarray(goal, np.float32)
    n, P = goal.shape
    _, scene = plan_scene(walls, hazards)
    if clearance is not None:
        reach, weight = plan_clearance_check(clearance)
    occ = grid_occupancy(spec, walls, hazards) if occupancy is None else occupancy
    field_of, fcell, fscene = plan_fields(spec, occ, scene, goal)
    if clearance is not None:
        clear = np.stack([grid_clearance(occ[s], reach) for s in range(len(occ))])
        pen = np.stack([grid_surcharge(occ[s], reach, weight) for s in range(len(occ))])
        clearance_min = np.full(n, -1, np.int32)
    if fields is None and clearance is None:
        fields = np.stack([grid_field(occ[fscene[f]], fcell[f]) for f in range(len(fcell))])
    elif fields is None:
        fields = np.stack([grid_field_cost(occ[fscene[f]], pen[fscene[f]], fcell[f]) for f in range(len(fcell))])
    wp, count, status, cost = np.zeros((n, K, P), np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    moves = np.zeros(n, np.int32)
    blocked = [los_blocked(occ[s], margin) for s in range(len(occ))] if smooth else None
    for i in range(n):
        f = field_of[i]
        walk = None
        if clearance is not None:
            walk = grid_walk_cost(fields[f], occ[fscene[f]], pen[fscene[f]], spec, start[i], goal[i])
            clearance_min[i] = grid_walk_clearance(walk, clear[fscene[f]], reach)
        if smooth:
            w, count[i], status[i], cost[i], moves[i] = grid_path_smooth(fields[f], occ[fscene[f]], spec, start[i], goal[i], K, margin,
                                                                         blocked[fscene[f]], walk)
        else:
            w, count[i], status[i], cost[i] = grid_path(fields[f], occ[fscene[f]], spec, start[i], goal[i], K, walk)
        m = min(int(count[i]), K)
        wp[i, :m, :2] = w[:m]
        wp[i, :m, 2:] = goal[i, 2:]
    out = {"waypoints": wp, "n_waypoints": np.minimum(count, K).astype(np.int32), "count": count, "status": status, "cost": cost,
           "occupancy": occ, "fields": fields, "field_of": field_of, "field_goal_cell": fcell, "field_scene": fscene}
    if smooth:
        out["moves"] = moves
    if clearance is not None:
        out["surcharge"], out["clearance_min"] = pen, clearance_min
    return out


# ---- clearance-aware plans: a per-cell surcharge near blocked cells.  This project's own rule, all integers; the
# device (csrc/kernels_plan.h: k_plan_surcharge, k_plan_field_cost, k_plan_path_cost, k_plan_smooth_cost) is held to it bit for bit.
# Entering a free cell c' costs the move plus pen[c'] = weight * max(0, reach + 1 - clearance[c']), where clearance is the Chebyshev
# distance in cells to the nearest blocked cell of the grid.  NOT promised: the plan is no longer the shortest; a doorway narrower
# than 2 * reach cells is still used (its surcharge is simply paid); `cost` includes the surcharges paid, `moves` stays the walk's
# length.  Only the static plan takes surcharges.
PLAN_CLEAR_REACH_MAX = 8
PLAN_CLEAR_WEIGHT_MAX = 16    # the largest surcharge is 16 * 8 = 128: a byte; a path costs at most G * G * (7 + 128), far below 2^30


def plan_clearance_check(clearance):
    """(reach, weight) -> the two as ints: reach 1 .. PLAN_CLEAR_REACH_MAX, weight 1 .. PLAN_CLEAR_WEIGHT_MAX, integers and not bools
    (ValueError naming `clearance` otherwise)"""
    try:
        reach, weight = clearance
    except (TypeError, ValueError):
        raise ValueError(f"clearance must be None or (reach, weight), got {clearance!r}") from None
    for name, v, top in (("reach", reach, PLAN_CLEAR_REACH_MAX), ("weight", weight, PLAN_CLEAR_WEIGHT_MAX)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= int(v) <= top:
            raise ValueError(f"clearance {name} must be an integer in 1 .. {top}, got {v!r}")
    return int(reach), int(weight)


def grid_clearance(occ_scene, reach):
    """uint8 [G][G]: the Chebyshev distance in cells to the nearest blocked cell of the grid, capped at reach + 1; blocked cells are 0;
    cells outside the grid count as free, as in grid_dilate.  `reach` rounds of grid_dilate: a cell's clearance is the first round
    that reaches it."""
    reach = plan_clearance_check((reach, 1))[0]
    grown = np.asarray(occ_scene, bool)
    out = np.where(grown, 0, reach + 1).astype(np.uint8)
    for r in range(1, reach + 1):
        nxt = grid_dilate(grown)
        out[nxt & ~grown] = r
        grown = nxt
    return out


def grid_surcharge(occ_scene, reach, weight):
    """uint8 [G][G]: weight * max(0, reach + 1 - grid_clearance) on free cells, 0 on blocked ones"""
    reach, weight = plan_clearance_check((reach, weight))
    clear = grid_clearance(occ_scene, reach).astype(np.int64)
    return np.where(np.asarray(occ_scene, bool), 0, weight * np.maximum(0, reach + 1 - clear)).astype(np.uint8)


def grid_field_cost(occ_scene, pen, goal_cell):
    """grid_field with the cost of a move k from c into c' being PLAN_STEP | PLAN_DIAG plus pen[c'] (pen uint8 [G][G]): int32 [G][G],
    the unique fixed point of d[c] = min_k(w(k) + pen[c'] + d[c']) under plan_move_ok with d[goal] = 0; -1 for blocked and
    unreachable cells, all -1 for a blocked goal cell.  The goal cell's own surcharge is paid on entry like any cell's; the cell a
    path starts in is never paid for.  Dijkstra from the goal: a cell c popped with d[c] offers d[c] + w + pen[c] to its neighbours
    (plan_move_ok is symmetric in the two cells)."""
    import heapq
    occ, pen = np.asarray(occ_scene, bool), np.asarray(pen).astype(np.int64)
    G = occ.shape[0]
    d = np.full((G, G), -1, np.int32)
    gx, gy = int(goal_cell) % G, int(goal_cell) // G
    if not 0 <= int(goal_cell) < G * G:
        raise ValueError(f"goal cell must lie in 0 .. {G * G - 1}, got {goal_cell}")
    if occ[gy, gx]:
        return d
    d[gy, gx] = 0
    heap = [(0, gy, gx)]
    while heap:
        dc, iy, ix = heapq.heappop(heap)
        if dc != d[iy, ix]:
            continue
        for k, (dx, dy) in enumerate(PLAN_DIRS):
            if plan_move_ok(occ, ix, iy, k):
                nd = dc + (PLAN_STEP if k < 4 else PLAN_DIAG) + int(pen[iy, ix])
                if d[iy + dy, ix + dx] < 0 or nd < d[iy + dy, ix + dx]:
                    d[iy + dy, ix + dx] = nd
                    heapq.heappush(heap, (nd, iy + dy, ix + dx))
    return d


def grid_walk_cost(field, occ_scene, pen, spec, start_xy, goal_xy):
    """grid_walk on a grid_field_cost field: the step goes to the allowed neighbour c' that minimises w(k) + pen[c'] + field[c'] --
    on such a field that minimum is field[c] -- under grid_walk's tie order: the previous direction if it attains it, else the
    lowest index of PLAN_DIRS -> (cells, directions, status) as grid_walk's."""
    occ, d, pen = np.asarray(occ_scene, bool), np.asarray(field), np.asarray(pen).astype(np.int64)
    G = spec.cells
    sx, sy = (int(v) for v in spec.cell_of(np.asarray(start_xy, np.float32)[:2]))
    gx, gy = (int(v) for v in spec.cell_of(np.asarray(goal_xy, np.float32)[:2]))
    if occ[sy, sx] or occ[gy, gx] or d[sy, sx] < 0:
        return [], [], UNREACHABLE
    cells, dirs, prev = [(sx, sy)], [], -1
    ix, iy = sx, sy
    while (ix, iy) != (gx, gy):
        def descends(k):
            jx, jy = ix + PLAN_DIRS[k][0], iy + PLAN_DIRS[k][1]
            return plan_move_ok(occ, ix, iy, k) and d[jy, jx] >= 0 and \
                d[jy, jx] + (PLAN_STEP if k < 4 else PLAN_DIAG) + pen[jy, jx] == d[iy, ix]
        k = prev if prev >= 0 and descends(prev) else next((j for j in range(8) if descends(j)), -1)
        if k < 0 or len(cells) > G * G:
            raise ValueError("grid_path_cost: the field is not the cost-to-go of this occupancy, surcharge and goal")
        ix, iy, prev = ix + PLAN_DIRS[k][0], iy + PLAN_DIRS[k][1], k
        cells.append((ix, iy))
        dirs.append(k)
    return cells, dirs, PLANNED


def grid_path_cost(field, occ_scene, pen, spec, start_xy, goal_xy, K):
    """grid_path on grid_walk_cost's walk: count, TRUNCATED, UNREACHABLE, the zeroed slots mean what they mean there; cost =
    field[start cell], the moves of the walk plus the surcharges of the cells it enters."""
    return grid_path(field, occ_scene, spec, start_xy, goal_xy, K, grid_walk_cost(field, occ_scene, pen, spec, start_xy, goal_xy))


def grid_walk_clearance(walk, clear, reach):
    """The least clearance (grid_clearance's map `clear`, capped at reach + 1) over the cells of a walk after its start cell; reach +
    1, the cap, for a walk of no moves (the start lies in the goal's cell); -1 without a walk (UNREACHABLE)."""
    cells, _, status = walk
    if status == UNREACHABLE:
        return -1
    return min([int(reach) + 1] + [int(clear[y, x]) for x, y in cells[1:]])


def grid_plan_clearance_min(spec, plan, start, goal, reach):
    """clearance_min [n] int32 of a PLAIN plan (grid_plan's or the planner's dict with occupancy and fields in it), recomputed from
    its walks with grid_walk_clearance: what a clearance-aware plan's clearance_min is compared with."""
    start, goal = np.asarray(start, np.float32), np.asarray(goal, np.float32)
    occ, out = np.asarray(plan["occupancy"], bool), np.zeros(len(goal), np.int32)
    clear = [grid_clearance(o, reach) for o in occ]
    for i, f in enumerate(plan["field_of"]):
        s = plan["field_scene"][f]
        out[i] = grid_walk_clearance(grid_walk(plan["fields"][f], occ[s], spec, start[i], goal[i]), clear[s], reach)
    return out


# ---- grid planner over time: moving hazards as LAYERS of occupancy, waits as release steps.  This project's own
# rule, integers but for grid_occupancy's floats; the device (csrc/kernels_plan.h: k_plan_occupancy_time, k_plan_field_time,
# k_plan_path_time) is held to it bit for bit.  A robot is given `layer_steps` steps for one action (a move or a wait); layer t < T
# covers the global steps step0 + t layer_steps .. step0 + (t + 1) layer_steps - 1, the tail layer T every step from step0 + T
# layer_steps on.  A layer's map blocks what ANY hazard frame in force during the layer blocks.
PLAN_WAIT = 4                     # cost of a wait: below a move's, so that two waits beat a step aside and back
PLAN_WAIT_ACTION = 8              # a wait in a walk's list of actions (0 .. 7: the moves of PLAN_DIRS)
PLAN_LAYERS_MAX = 256
PLAN_TIME_MAX_BYTES = 256 << 20   # cap on the time fields of one plan (F * (T + 1) * G * G * 4 bytes); the engine refuses more too


def plan_scene_time(walls, hazards):
    """plan_scene for a time plan: hazards must be a MovingHazards -> (S, scene [n] int32 or None)"""
    if walls is not None and not isinstance(walls, Walls):
        raise TypeError(f"walls must be a mobrob_amd.envs.goal_rules.Walls, not {type(walls).__name__}")
    if not isinstance(hazards, MovingHazards):
        raise TypeError(f"a time plan needs hazards that are a mobrob_amd.envs.goal_rules.MovingHazards, not {type(hazards).__name__}")
    return _scene_agreement(walls, hazards)


def plan_time_check(step0, layer_steps, layers):
    """-> (step0, layer_steps, layers) as ints, or ValueError: step0 >= 0, layer_steps >= 1, 1 <= layers <= PLAN_LAYERS_MAX, and
    the first step of the layer after the tail's first, step0 + (layers + 1) * layer_steps, fits an int32"""
    for name, v in (("step0", step0), ("layer_steps", layer_steps), ("layers", layers)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"plan_time: {name} must be an integer, got {v!r}")
    step0, layer_steps, layers = int(step0), int(layer_steps), int(layers)
    if step0 < 0:
        raise ValueError(f"plan_time: step0 must be >= 0, got {step0}")
    if layer_steps < 1:
        raise ValueError(f"plan_time: layer_steps must be >= 1, got {layer_steps}")
    if not 1 <= layers <= PLAN_LAYERS_MAX:
        raise ValueError(f"plan_time: layers must lie in 1 .. {PLAN_LAYERS_MAX}, got {layers}")
    if step0 + (layers + 1) * layer_steps > 2 ** 31 - 1:
        raise ValueError(f"plan_time: step0 + (layers + 1) * layer_steps = {step0 + (layers + 1) * layer_steps} must fit an int32")
    return step0, layer_steps, layers


def grid_layer_frames(hazards, step0, layer_steps, layers):
    """The frames of every layer -> (first [T + 1] int32, number [T + 1] int32): layer t's set is the cyclically contiguous run of
    `number[t]` frames from `first[t]` (indices mod F).  With k(g) = g // frame_steps, layer t < T covers k_lo = k(step0 + t
    layer_steps) .. k_hi = k(step0 + (t + 1) layer_steps - 1): hold: frames min(k_lo, F - 1) .. min(k_hi, F - 1); loop: min(k_hi -
    k_lo + 1, F) frames from k_lo % F.  The tail: loop: all F frames from 0; hold: frame_index(step0 + T layer_steps) .. F - 1."""
    step0, layer_steps, layers = plan_time_check(step0, layer_steps, layers)
    F, fs = hazards.n_frames, hazards.frame_steps
    first, number = np.zeros(layers + 1, np.int32), np.zeros(layers + 1, np.int32)
    for t in range(layers):
        k_lo, k_hi = (step0 + t * layer_steps) // fs, (step0 + (t + 1) * layer_steps - 1) // fs
        if hazards.loop:
            first[t], number[t] = k_lo % F, min(k_hi - k_lo + 1, F)
        else:
            first[t] = min(k_lo, F - 1)
            number[t] = min(k_hi, F - 1) - first[t] + 1
    if hazards.loop:
        first[layers], number[layers] = 0, F
    else:
        first[layers] = min((step0 + layers * layer_steps) // fs, F - 1)
        number[layers] = F - first[layers]
    return first, number


def grid_occupancy_time(spec, walls, hazards, step0, layer_steps, layers):
    """bool [S][T + 1][G][G]: layer t blocks a cell that grid_occupancy blocks for the walls or for the hazard rows of ANY frame of
    the layer's set (grid_layer_frames): every position a hazard takes during the layer.  The tail is a conservative static scene."""
    S, _ = plan_scene_time(walls, hazards)
    first, number = grid_layer_frames(hazards, step0, layer_steps, layers)
    G, F = spec.cells, hazards.n_frames
    inflate = spec.inflate_for(walls)
    c = spec.centre(np.arange(G))
    px, py = np.broadcast_to(c[None, :], (G, G)), np.broadcast_to(c[:, None], (G, G))
    static = grid_occupancy(spec, walls, None) if walls is not None else np.zeros((S, G, G), bool)
    occ = np.zeros((S, len(first), G, G), bool)
    for s in range(S):
        frames = {}
        for t in range(len(first)):
            occ[s, t] = static[s]
            for j in range(int(number[t])):
                f = (int(first[t]) + j) % F
                if f not in frames:
                    frames[f] = _hazard_rows_block(px, py, hazards.table[s, f, :int(hazards.counts[s])], inflate)
                occ[s, t] |= frames[f]
    return occ


def plan_moves_ok(occ):
    """bool [8][G][G]: plan_move_ok(occ, ix, iy, k) of every cell at once (the value at a blocked cell has no meaning)"""
    occ = np.asarray(occ, bool)
    G = occ.shape[0]
    pad = np.ones((G + 2, G + 2), bool)
    pad[1:-1, 1:-1] = occ
    out = np.zeros((8, G, G), bool)
    for k, (dx, dy) in enumerate(PLAN_DIRS):
        out[k] = ~pad[1 + dy:1 + dy + G, 1 + dx:1 + dx + G]
        if k >= 4:
            out[k] &= ~pad[1:1 + G, 1 + dx:1 + dx + G] & ~pad[1 + dy:1 + dy + G, 1:1 + G]
    return out


def grid_time_field(occ_layers, goal_cell):
    """int32 [T + 1][G][G], the cost-to-go over moves and waits through the layers occ_layers [T + 1][G][G]: d_T = grid_field(occ_T,
    goal cell); for t = T - 1 .. 0, d_t[c] = -1 where occ_t blocks c, else 0 in the goal cell, else the minimum of d_{t+1}[nb] + w_k
    over the moves k with plan_move_ok(occ_t, c, k) and d_{t+1}[nb] >= 0 and of the wait d_{t+1}[c] + PLAN_WAIT where d_{t+1}[c] >=
    0; -1 when nothing qualifies.  Every layer is a pure function of the next one."""
    occ = np.asarray(occ_layers, bool)
    T, G = occ.shape[0] - 1, occ.shape[1]
    d = np.full((T + 1, G, G), -1, np.int32)
    d[T] = grid_field(occ[T], goal_cell)
    gx, gy = int(goal_cell) % G, int(goal_cell) // G
    big = np.int32(2 ** 30)
    for t in range(T - 1, -1, -1):
        nxt = np.full((G + 2, G + 2), -1, np.int32)
        nxt[1:-1, 1:-1] = d[t + 1]
        ok = plan_moves_ok(occ[t])
        best = np.where(d[t + 1] >= 0, d[t + 1] + np.int32(PLAN_WAIT), big)
        for k, (dx, dy) in enumerate(PLAN_DIRS):
            nb = nxt[1 + dy:1 + dy + G, 1 + dx:1 + dx + G]
            best = np.minimum(best, np.where(ok[k] & (nb >= 0), nb + np.int32(PLAN_STEP if k < 4 else PLAN_DIAG), big))
        best = np.where(best >= big, np.int32(-1), best)
        if not occ[t, gy, gx]:
            best[gy, gx] = 0
        d[t] = np.where(occ[t], np.int32(-1), best)
    return d


def grid_walk_time(field, occ_layers, spec, start_xy, goal_xy):
    """The walk of a time plan -> (cells [(ix, iy), ...] one per action plus the start's, actions [0 .. 7 a move of PLAN_DIRS,
    PLAN_WAIT_ACTION a wait], status): UNREACHABLE (empty lists) iff field[0][start cell] < 0.  While the walk is not in the goal's
    cell and t < T it takes the first that qualifies of: the previous move; the lowest move of PLAN_DIRS; the wait.  A move k
    qualifies when plan_move_ok(occ_t, c, k), d_{t+1}[nb] >= 0 and d_{t+1}[nb] + w_k == d_t[c]; the wait when d_{t+1}[c] >= 0 and
    d_{t+1}[c] + PLAN_WAIT == d_t[c].  A wait leaves the previous move alone; every action advances t by one.  From t = T on the
    walk is grid_walk's own step on (d_T, occ_T), the previous move carried in."""
    occ, d = np.asarray(occ_layers, bool), np.asarray(field)
    T, G = d.shape[0] - 1, spec.cells
    sx, sy = (int(v) for v in spec.cell_of(np.asarray(start_xy, np.float32)[:2]))
    gx, gy = (int(v) for v in spec.cell_of(np.asarray(goal_xy, np.float32)[:2]))
    if d[0, sy, sx] < 0:
        return [], [], UNREACHABLE
    cells, acts, prev = [(sx, sy)], [], -1
    ix, iy = sx, sy
    while (ix, iy) != (gx, gy):
        t = min(len(acts), T)
        nxt = d[min(t + 1, T)]

        def descends(k):
            jx, jy = ix + PLAN_DIRS[k][0], iy + PLAN_DIRS[k][1]
            return plan_move_ok(occ[t], ix, iy, k) and nxt[jy, jx] >= 0 and nxt[jy, jx] + (PLAN_STEP if k < 4 else PLAN_DIAG) == d[t, iy, ix]
        k = prev if prev >= 0 and descends(prev) else next((j for j in range(8) if descends(j)), -1)
        if k < 0 and t < T and nxt[iy, ix] >= 0 and nxt[iy, ix] + PLAN_WAIT == d[t, iy, ix]:
            k = PLAN_WAIT_ACTION
        if k < 0 or len(acts) >= T + G * G:
            raise ValueError("grid_walk_time: the field is not the time field of these layers and this goal")
        if k != PLAN_WAIT_ACTION:
            ix, iy, prev = ix + PLAN_DIRS[k][0], iy + PLAN_DIRS[k][1], k
        cells.append((ix, iy))
        acts.append(k)
    return cells, acts, PLANNED


def grid_path_time(field, occ_layers, spec, start_xy, goal_xy, K):
    """One robot's time plan -> (waypoints [K][2] float32, count, status, cost, waits [K] int32, leave [K] int32, arrive).  A cell the
    walk entered by a move is a waypoint when the move leaving it differs from the move entering it, or when the walk waited there;
    the start cell emits nothing; the last waypoint is goal_xy itself.  count, the first min(count, K) slots, TRUNCATED and cost =
    field[0][start cell] as in grid_path.  waits[k]: the waits made at waypoint k's ANCHOR (the previous waypoint's cell, the start
    cell for k = 0); leave[k]: the actions made before the move that leaves that anchor; arrive: the actions of the whole walk."""
    K = int(K)
    if K < 1:
        raise ValueError("max_waypoints must be >= 1")
    wp, waits, leave = np.zeros((K, 2), np.float32), np.zeros(K, np.int32), np.zeros(K, np.int32)
    cells, acts, status = grid_walk_time(field, occ_layers, spec, start_xy, goal_xy)
    if status == UNREACHABLE:
        return wp, 0, UNREACHABLE, -1, waits, leave, 0
    count, prev, waited = 0, -1, 0
    for a, k in enumerate(acts):
        if k == PLAN_WAIT_ACTION:
            waited += 1
            continue
        turned = prev >= 0 and (k != prev or waited > 0)
        if turned:
            if count < K:
                wp[count] = spec.centre(cells[a][0]), spec.centre(cells[a][1])
            count += 1
        if (prev < 0 or turned) and count < K:      # this move leaves the anchor of waypoint `count`
            waits[count], leave[count] = waited, a
        prev, waited = k, 0
    if count < K:
        wp[count] = np.asarray(goal_xy, np.float32)[:2]
    count += 1
    sx, sy = cells[0]
    return wp, count, TRUNCATED if count > K else PLANNED, int(np.asarray(field)[0, sy, sx]), waits, leave, len(acts)


def grid_release(waits, leave, step0, layer_steps):
    """Schedule's release steps of a time plan, int32 like `waits`: step0 + leave * layer_steps where waits > 0, else 0 -- the
    hold at waypoint k's anchor (for k = 0: at `home`, the start) until the move that leaves it"""
    waits, leave = np.asarray(waits, np.int64), np.asarray(leave, np.int64)
    return np.where(waits > 0, int(step0) + leave * int(layer_steps), 0).astype(np.int32)


def plan_time_smooth_check(n_fields, n_scenes, layers, cells, margin):
    """ValueError unless margin is 0 or 1 and the time fields plus the next-blocked table (n_scenes * (layers + 1) * cells^2 * 2
    bytes) stay within PLAN_TIME_MAX_BYTES; the engine refuses the same"""
    if isinstance(margin, bool) or margin not in (0, 1):
        raise ValueError(f"line-of-sight margin must be 0 or 1, got {margin!r}")
    if (n_fields * 4 + n_scenes * 2) * (layers + 1) * cells ** 2 > PLAN_TIME_MAX_BYTES:
        raise ValueError(f"plan_time: time fields of {n_fields} x {layers + 1} x {cells} x {cells} x 4 bytes and the next-blocked table of "
                         f"{n_scenes} x {layers + 1} x {cells} x {cells} x 2 bytes exceed the cap of {PLAN_TIME_MAX_BYTES} bytes "
                         f"({PLAN_TIME_MAX_BYTES >> 20} MiB)")


def grid_plan_time(spec, walls, hazards, start, goal, K, step0=0, layer_steps=1, layers=64, smooth=False, margin=1,
                   want_next_blocked=False):
    """The whole time plan of n robots by the rule: grid_plan's dict with occupancy bool [S][T + 1][G][G] and fields int32 [F][T +
    1][G][G] (fields numbered as plan_fields numbers them), plus waits, leave [n][K] int32, arrive [n] int32, release [n][K] int32
    (grid_release) and layer_first, layer_number [T + 1] (grid_layer_frames).  smooth: the paths by grid_path_smooth_time with the
    line-of-sight `margin` (0 or 1): waypoints, n_waypoints, count, status and leave are the smoothed plan's, release is
    grid_release_smooth's (a hold at every anchor but the start), waits is all zero, `moves` [n] int32 joins them, and with
    want_next_blocked `next_blocked` int16 [S][T + 1][G][G] (grid_next_blocked of every scene)."""
    start, goal = np.asarray(start, np.float32), np.asarray(goal, np.float32)
    n, P = goal.shape
    S, scene = plan_scene_time(walls, hazards)
    step0, layer_steps, layers = plan_time_check(step0, layer_steps, layers)
    field_of, fcell, fscene = plan_fields(spec, None, scene, goal)
    if smooth:
        plan_time_smooth_check(len(fcell), S, layers, spec.cells, margin)
    if len(fcell) * (layers + 1) * spec.cells ** 2 * 4 > PLAN_TIME_MAX_BYTES:
        raise ValueError(f"plan_time: time fields of {len(fcell)} x {layers + 1} x {spec.cells} x {spec.cells} x 4 bytes exceed the cap of "
                         f"{PLAN_TIME_MAX_BYTES} bytes ({PLAN_TIME_MAX_BYTES >> 20} MiB)")
    first, number = grid_layer_frames(hazards, step0, layer_steps, layers)
    occ = grid_occupancy_time(spec, walls, hazards, step0, layer_steps, layers)
    fields = np.stack([grid_time_field(occ[fscene[f]], fcell[f]) for f in range(len(fcell))])
    wp, waits, leave = np.zeros((n, K, P), np.float32), np.zeros((n, K), np.int32), np.zeros((n, K), np.int32)
    count, status, cost, arrive, moves = (np.zeros(n, np.int32) for _ in range(5))
    nb = np.stack([grid_next_blocked([los_blocked(o, margin) for o in occ[s]]) for s in range(S)]) if smooth else None
    for i in range(n):
        f = field_of[i]
        if smooth:
            w, count[i], status[i], cost[i], leave[i], arrive[i], moves[i] = grid_path_smooth_time(
                fields[f], occ[fscene[f]], spec, start[i], goal[i], K, margin, nb[fscene[f]])
        else:
            w, count[i], status[i], cost[i], waits[i], leave[i], arrive[i] = grid_path_time(fields[f], occ[fscene[f]], spec, start[i], goal[i], K)
        m = min(int(count[i]), K)
        wp[i, :m, :2] = w[:m]
        wp[i, :m, 2:] = goal[i, 2:]
    out = {"waypoints": wp, "n_waypoints": np.minimum(count, K).astype(np.int32), "count": count, "status": status, "cost": cost,
           "waits": waits, "leave": leave, "arrive": arrive,
           "release": grid_release_smooth(leave, step0, layer_steps) if smooth else grid_release(waits, leave, step0, layer_steps),
           "occupancy": occ, "fields": fields, "field_of": field_of, "field_goal_cell": fcell, "field_scene": fscene,
           "layer_first": first, "layer_number": number}
    if smooth:
        out["moves"] = moves
        if want_next_blocked:
            out["next_blocked"] = nb
    return out


# ---- line-of-sight smoothing of a time plan: a straight leg is tested against EVERY layer it spans.  All integers;
# the device (csrc/kernels_plan.h: k_plan_next_blocked, k_plan_smooth_time) is held to it bit for bit.  A kept leg from action index
# a to b with b - a >= 2: every cell of the supercover between c[a] and c[b], both ends included, is clear at the margin in each of
# the layers min(a, T) .. min(b, T) -- whatever the robot's speed along the leg, as long as it leaves c[a] no earlier and reaches c[b]
# no later than the walk does.  A leg of one action is the walk's own action and carries grid_walk_time's promise only.
PLAN_NEVER_BLOCKED = 32767   # grid_next_blocked's "in no layer from here on" (PLAN_LAYERS_MAX is 256: int16 holds every layer)


def grid_next_blocked(blk_layers):
    """int16 [T + 1][G][G] of the maps blk_layers [T + 1][G][G] (los_blocked of every layer): nb[t][c] is the first layer from t on
    in which c is not clear, PLAN_NEVER_BLOCKED where there is none.  nb[T][c] = T if blk_T[c] else PLAN_NEVER_BLOCKED; for t = T -
    1 .. 0, nb[t][c] = t if blk_t[c] else nb[t + 1][c].  So c is clear in all of the layers lo .. hi (lo <= hi <= T) exactly when
    nb[lo][c] > hi: one load per cell per test, whatever the span."""
    blk = np.asarray(blk_layers, bool)
    T = blk.shape[0] - 1
    nb = np.empty(blk.shape, np.int16)
    nb[T] = np.where(blk[T], np.int16(T), np.int16(PLAN_NEVER_BLOCKED))
    for t in range(T - 1, -1, -1):
        nb[t] = np.where(blk[t], np.int16(t), nb[t + 1])
    return nb


def plan_max_leg_check(max_leg):
    """-> max_leg as an int, or ValueError: the cap on a smoothed leg's length in actions, an integer >= 1"""
    if isinstance(max_leg, bool) or not isinstance(max_leg, (int, np.integer)) or int(max_leg) < 1:
        raise ValueError(f"plan_team: max_leg must be an integer >= 1 (None: no cap), got {max_leg!r}")
    return int(max_leg)


class _SpanBlocked:
    """the map `nb[lo] <= hi` of grid_los_time, a cell at a time (los_walk reads blk[y, x])"""

    def __init__(self, nb, lo, hi):
        self.row, self.hi = nb[lo], hi

    def __getitem__(self, yx):
        return self.row[yx] <= self.hi


def grid_los_time(nb, a, b, lo, hi):
    """Is cell b visible from cell a in every layer lo .. hi (lo <= hi <= T)?  los_walk on the map nb[lo] <= hi: the same
    supercover, the same t == 0 corner rule, false if a is not clear; symmetric in a and b."""
    return los_walk(_SpanBlocked(nb, int(lo), int(hi)), a, b)[0]


def grid_smooth_time(cells, nb, max_leg=None):
    """Line-of-sight smoothing of grid_walk_time's cells c[0 .. A] (one per action boundary, a wait repeats its cell) -> the ascending
    action indices kept as waypoints.  T = nb.shape[0] - 1.  Anchor i = 0, j = 1; while j < A: if grid_los_time(nb, c[i], c[j + 1],
    min(i, T), min(j + 1, T)) then j += 1, else emit j, i = j, j += 1.  A leg of one action is never tested.  Waits are not special:
    a leg that is clear through all its layers may skip a cell where the walk waited (the robot holds at the leg's anchor instead:
    grid_release_smooth).  max_leg (None: no cap, an integer >= 1 otherwise): the leg from c[i] to c[j + 1] is kept only if it is
    clear AND j + 1 - i <= max_leg actions long; max_leg = 1 keeps every cell of the walk."""
    if max_leg is not None:
        max_leg = plan_max_leg_check(max_leg)
    A, T, out, i, j = len(cells) - 1, nb.shape[0] - 1, [], 0, 1
    while j < A:
        if (max_leg is not None and j + 1 - i > max_leg) or not grid_los_time(nb, cells[i], cells[j + 1], min(i, T), min(j + 1, T)):
            out.append(j)
            i = j
        j += 1
    return out


def grid_path_smooth_time(field, occ_layers, spec, start_xy, goal_xy, K, margin=1, nb=None):
    """grid_path_time with line-of-sight smoothing -> (waypoints [K][2] float32, count, status, cost, leave [K] int32, arrive, moves):
    the waypoints are the centres of the cells grid_smooth_time keeps of the walk, then goal_xy itself; count, the first min(count,
    K) slots, the zeroed slots, TRUNCATED, UNREACHABLE and cost = field[0][start cell] mean what they mean in grid_path_time.
    leave[k]: the action index of waypoint k's anchor, 0 for k = 0 and the kept index of waypoint k - 1 otherwise; arrive = A, the
    actions of the walk; moves: those of them that are moves.  nb: grid_next_blocked of the scene's layers at this margin,
    computed once by a caller with many walks."""
    K = int(K)
    if K < 1:
        raise ValueError("max_waypoints must be >= 1")
    wp, leave = np.zeros((K, 2), np.float32), np.zeros(K, np.int32)
    cells, acts, status = grid_walk_time(field, occ_layers, spec, start_xy, goal_xy)
    if status == UNREACHABLE:
        return wp, 0, UNREACHABLE, -1, leave, 0, 0
    if nb is None:
        nb = grid_next_blocked([los_blocked(o, margin) for o in np.asarray(occ_layers, bool)])
    keep = grid_smooth_time(cells, nb)
    for count, j in enumerate(keep[:K]):
        wp[count] = spec.centre(cells[j][0]), spec.centre(cells[j][1])
    count = len(keep)
    if count < K:
        wp[count] = np.asarray(goal_xy, np.float32)[:2]
    count += 1
    leave[1:min(count, K)] = keep[:min(count, K) - 1]
    sx, sy = cells[0]
    return (wp, count, TRUNCATED if count > K else PLANNED, int(np.asarray(field)[0, sy, sx]), leave, len(acts),
            sum(k != PLAN_WAIT_ACTION for k in acts))


def grid_release_smooth(leave, step0, layer_steps):
    """Schedule's release steps of a smoothed time plan, int32: step0 + leave * layer_steps where leave > 0, else 0 -- a hold at
    EVERY anchor but the start, not only where the walk waited: a straight leg is shorter than the walk it replaces, so the robot
    arrives early and must not enter the next leg before the first layer that leg was tested in.  ValueError where a release step
    does not fit an int32."""
    leave = np.asarray(leave, np.int64)
    release = np.where(leave > 0, int(step0) + leave * int(layer_steps), 0)
    if release.size and release.max() > 2 ** 31 - 1:
        raise ValueError(f"plan_time: a release step of {int(release.max())} must fit an int32")
    return release.astype(np.int32)


# ---- prioritised planning inside a team: a mate's planned walk is one more moving obstacle in the layers.  This
# project's own rule, integers but for the occupancy's floats; the device (csrc/kernels_plan.h: k_plan_team) is held to it bit for
# bit.  The member with team-local index m plans after the members 0 .. m - 1 on occ_t = base_t OR res_t, res the union of their
# reservations; teams never see each other.  Prioritised planning is INCOMPLETE: inside one plan a member never yields to a later
# one (grid_plan_team_rounds, further down, plans a team again with the members that stayed parked first).
PLAN_RESERVE_MAX = 4
PLAN_NO_PAIR = 2 ** 31 - 1        # the clearance of a team without a pair of mates (size 1)


def plan_team_check(teams, reserve, n, scene=None):
    """-> (size, reserve) as ints, or ValueError: teams a Teams whose size divides n, reserve an integer in 0 .. PLAN_RESERVE_MAX,
    all members of a team in one scene"""
    if not isinstance(teams, Teams):
        raise TypeError(f"teams must be a mobrob_amd.envs.goal_rules.Teams, not {type(teams).__name__}")
    teams.check_robots(n)
    if isinstance(reserve, bool) or not isinstance(reserve, (int, np.integer)) or not 0 <= int(reserve) <= PLAN_RESERVE_MAX:
        raise ValueError(f"plan_team: reserve must be an integer in 0 .. {PLAN_RESERVE_MAX}, got {reserve!r}")
    if scene is not None:
        sc = np.asarray(scene).reshape(-1, teams.size)
        if np.any(sc != sc[:, :1]):
            raise ValueError(f"plan_team: all members of a team must be in one scene (team {int(np.nonzero(np.any(sc != sc[:, :1], axis=1))[0][0])} is not)")
    return teams.size, int(reserve)


def plan_team_reserve(teams, spec):
    """The default reserve of a planner: ceil(separation / h), the smallest r for which centres more than r cells apart are at least
    separation + h apart along an axis; ValueError above PLAN_RESERVE_MAX"""
    r = int(np.ceil(float(teams.separation) / float(spec.h)))
    if r > PLAN_RESERVE_MAX:
        raise ValueError(f"plan_team: a separation of {teams.separation} needs reserve = {r} cells of {float(spec.h)}, at most {PLAN_RESERVE_MAX}: use a coarser grid")
    return r


def plan_team_base(spec, walls, hazards, step0, layer_steps, layers):
    """The base layers of a team plan, bool [S][T + 1][G][G] -> (occupancy, S, scene): grid_occupancy's map in every layer for None and
    Hazards (a team plan is a time plan even in a static scene), grid_occupancy_time's for MovingHazards"""
    if isinstance(hazards, MovingHazards):
        S, scene = plan_scene_time(walls, hazards)
        return grid_occupancy_time(spec, walls, hazards, step0, layer_steps, layers), S, scene
    S, scene = plan_scene(walls, hazards)
    occ = grid_occupancy(spec, walls, hazards)
    return np.ascontiguousarray(np.broadcast_to(occ[:, None], (S, layers + 1) + occ.shape[1:])), S, scene


def grid_reserve(walk, layers, G, reserve):
    """The reservation of a walk with cells c[0 .. A] (c[a] = c[A] beyond), bool [T + 1][G][G]: layer t < T reserves every cell within
    Chebyshev distance `reserve` of c[t] or c[t + 1], the tail layer T every cell within it of any c[a], a >= min(T, A)."""
    T, r, A = int(layers), int(reserve), len(walk) - 1
    res = np.zeros((T + 1, G, G), bool)

    def stamp(t, c):
        res[t, max(c[1] - r, 0):c[1] + r + 1, max(c[0] - r, 0):c[0] + r + 1] = True
    for t in range(T):
        stamp(t, walk[min(t, A)])
        stamp(t, walk[min(t + 1, A)])
    for a in range(min(T, A), A + 1):
        stamp(T, walk[a])
    return res


def grid_team_field(occ_layers, goal_cell):
    """grid_time_field with one change: the goal cell is terminal (d_t = 0) only where it is free in occ_t AND in every later layer up
    to T; otherwise it is an ordinary cell, so a robot may wait on it or step off and come back."""
    occ = np.asarray(occ_layers, bool)
    T, G = occ.shape[0] - 1, occ.shape[1]
    d = np.full((T + 1, G, G), -1, np.int32)
    d[T] = grid_field(occ[T], goal_cell)
    gx, gy = int(goal_cell) % G, int(goal_cell) // G
    big = np.int32(2 ** 30)
    terminal = not occ[T, gy, gx]
    for t in range(T - 1, -1, -1):
        terminal = terminal and not occ[t, gy, gx]
        nxt = np.full((G + 2, G + 2), -1, np.int32)
        nxt[1:-1, 1:-1] = d[t + 1]
        ok = plan_moves_ok(occ[t])
        best = np.where(d[t + 1] >= 0, d[t + 1] + np.int32(PLAN_WAIT), big)
        for k, (dx, dy) in enumerate(PLAN_DIRS):
            nb = nxt[1 + dy:1 + dy + G, 1 + dx:1 + dx + G]
            best = np.minimum(best, np.where(ok[k] & (nb >= 0), nb + np.int32(PLAN_STEP if k < 4 else PLAN_DIAG), big))
        best = np.where(best >= big, np.int32(-1), best)
        if terminal:
            best[gy, gx] = 0
        d[t] = np.where(occ[t], np.int32(-1), best)
    return d


def grid_walk_team(field, occ_layers, spec, start_xy):
    """grid_walk_time with one change: the walk ends when d_t[c] == 0 (a terminal goal cell), not on entering the goal's cell."""
    occ, d = np.asarray(occ_layers, bool), np.asarray(field)
    T, G = d.shape[0] - 1, spec.cells
    ix, iy = (int(v) for v in spec.cell_of(np.asarray(start_xy, np.float32)[:2]))
    if d[0, iy, ix] < 0:
        return [], [], UNREACHABLE
    cells, acts, prev = [(ix, iy)], [], -1
    while d[min(len(acts), T), iy, ix] != 0:
        t = min(len(acts), T)
        nxt = d[min(t + 1, T)]

        def descends(k):
            jx, jy = ix + PLAN_DIRS[k][0], iy + PLAN_DIRS[k][1]
            return plan_move_ok(occ[t], ix, iy, k) and nxt[jy, jx] >= 0 and nxt[jy, jx] + (PLAN_STEP if k < 4 else PLAN_DIAG) == d[t, iy, ix]
        k = prev if prev >= 0 and descends(prev) else next((j for j in range(8) if descends(j)), -1)
        if k < 0 and t < T and nxt[iy, ix] >= 0 and nxt[iy, ix] + PLAN_WAIT == d[t, iy, ix]:
            k = PLAN_WAIT_ACTION
        if k < 0 or len(acts) >= T + G * G:
            raise ValueError("grid_walk_team: the field is not the team field of these layers and this goal")
        if k != PLAN_WAIT_ACTION:
            ix, iy, prev = ix + PLAN_DIRS[k][0], iy + PLAN_DIRS[k][1], k
        cells.append((ix, iy))
        acts.append(k)
    return cells, acts, PLANNED


def grid_path_team(field, occ_layers, spec, start_xy, goal_xy, K):
    """grid_path_time on grid_walk_team's walk -> (grid_path_time's tuple, cells of the walk ([] when UNREACHABLE))"""
    K = int(K)
    if K < 1:
        raise ValueError("max_waypoints must be >= 1")
    wp, waits, leave = np.zeros((K, 2), np.float32), np.zeros(K, np.int32), np.zeros(K, np.int32)
    cells, acts, status = grid_walk_team(field, occ_layers, spec, start_xy)
    if status == UNREACHABLE:
        return (wp, 0, UNREACHABLE, -1, waits, leave, 0), []
    count, prev, waited = 0, -1, 0
    for a, k in enumerate(acts):
        if k == PLAN_WAIT_ACTION:
            waited += 1
            continue
        turned = prev >= 0 and (k != prev or waited > 0)
        if turned:
            if count < K:
                wp[count] = spec.centre(cells[a][0]), spec.centre(cells[a][1])
            count += 1
        if (prev < 0 or turned) and count < K:      # this move leaves the anchor of waypoint `count`
            waits[count], leave[count] = waited, a
        prev, waited = k, 0
    if count < K:
        wp[count] = np.asarray(goal_xy, np.float32)[:2]
    count += 1
    sx, sy = cells[0]
    return (wp, count, TRUNCATED if count > K else PLANNED, int(np.asarray(field)[0, sy, sx]), waits, leave, len(acts)), cells


def grid_team_clearance(walks, size, layers=None):
    """The checker of a team plan, independent of the planner: it sees walks only, never occupancy or fields.  walks: per robot the
    cells [(ix, iy), ...] c[0 .. A] of its walk (c[a] = c[A] beyond; a parked robot: its start cell alone), robots i and j mates when
    i // size == j // size -> (clearance [n_teams] int32, crossings [n_teams] int32).  clearance: the smallest Chebyshev cell distance
    of two mates over, for every action t < T, the four pairs {c_i[t], c_i[t + 1]} x {c_j[t], c_j[t + 1]}, and over every pair c_i[a],
    c_j[b] of the tails, a >= min(T, A_i), b >= min(T, A_j); PLAN_NO_PAIR for a team of one.  crossings: the actions t in which two
    mates both move diagonally inside one 2 x 2 block, across each other.  layers = T, the layers of the plan: pass it to check what
    the rule guarantees.  None takes T beyond every walk: every action is then checked in step and the tails are the last cells
    alone, which is less than the guarantee for walks that run on into the tail layer."""
    n = len(walks)
    lengths = np.array([len(w) for w in walks], np.int64)
    if n and lengths.min() < 1:
        raise ValueError("grid_team_clearance: every walk has at least its start cell")
    cells = np.zeros((n, max(int(lengths.max()), 1) if n else 1, 2), np.int64)
    for i, w in enumerate(walks):
        cells[i, :lengths[i]] = np.asarray(w, np.int64).reshape(-1, 2)
    return grid_team_clearance_cells(cells, lengths, size, layers)


def grid_team_clearance_cells(cells, lengths, size, layers=None):
    """grid_team_clearance on arrays: cells [n][L][2] (ix, iy), robot i's walk in its first lengths[i] >= 1 entries.  All pairs of
    mates and all teams at once; the tails pair by pair only where a walk runs on into the tail layer."""
    cells, lengths, size = np.asarray(cells, np.int64), np.asarray(lengths, np.int64), int(size)
    n = cells.shape[0]
    if size < 1 or n % size != 0:
        raise ValueError(f"{n} walks do not split into teams of {size}")
    if n and (lengths.min() < 1 or lengths.max() > cells.shape[1]):
        raise ValueError("grid_team_clearance: every walk has at least its start cell")
    g = n // size
    T = int(lengths.max()) if layers is None else int(layers)
    clear, cross = np.full(g, PLAN_NO_PAIR, np.int64), np.zeros(g, np.int64)
    if size == 1 or n == 0:
        return clear.astype(np.int32), cross.astype(np.int32)
    idx = np.minimum(np.arange(T + 2)[None, :], lengths[:, None] - 1)                # c[0 .. T + 1], padded with c[A]
    c = cells[np.arange(n)[:, None], idx].reshape(g, size, T + 2, 2)
    pair = np.triu(np.ones((size, size), bool), 1)[None, :, :, None]                 # i < j
    big = np.int64(PLAN_NO_PAIR)
    if T > 0:
        for p in (c[:, :, None, :T], c[:, :, None, 1:T + 1]):
            for q in (c[:, None, :, :T], c[:, None, :, 1:T + 1]):
                dist = np.where(pair, np.abs(p - q).max(axis=-1), big)               # [g][size][size][T]
                clear = np.minimum(clear, dist.min(axis=(1, 2, 3)))
        move = c[:, :, 1:T + 1] - c[:, :, :T]
        diag = np.abs(move).sum(axis=-1) == 2                                         # [g][size][T]
        low = np.minimum(c[:, :, :T], c[:, :, 1:T + 1])                              # the block's lower-left corner
        # both diagonals of one block: the two moves share the corner and neither start is the other's start or end
        hit = (diag[:, :, None] & diag[:, None, :] & np.all(low[:, :, None] == low[:, None, :], axis=-1)
               & np.any(c[:, :, None, :T] != c[:, None, :, :T], axis=-1) & np.any(c[:, :, None, :T] != c[:, None, :, 1:T + 1], axis=-1))
        cross = (hit & pair).sum(axis=(1, 2, 3))
    # the tails: c[min(T, A) .. A]; one cell for a walk that ends before the tail layer
    first = np.minimum(T, lengths - 1)
    one = cells[np.arange(n), first].reshape(g, size, 2)
    short = (lengths - first == 1).reshape(g, size)
    dist = np.where(pair[..., 0] & short[:, :, None] & short[:, None, :], np.abs(one[:, :, None] - one[:, None, :]).max(axis=-1), big)
    clear = np.minimum(clear, dist.min(axis=(1, 2)))
    for i in np.flatnonzero(~short.ravel()):                                          # a long tail against each mate's tail
        ti = cells[i, first[i]:lengths[i]]
        for j in range(i // size * size, (i // size + 1) * size):
            if j != i and (j > i or short.ravel()[j]):
                tj = cells[j, first[j]:lengths[j]]
                clear[i // size] = min(clear[i // size], int(np.abs(ti[:, None, :] - tj[None, :, :]).max(axis=2).min()))
    return clear.astype(np.int32), cross.astype(np.int32)


def grid_leg_cells(a, b):
    """The cells los_walk visits between cell a and cell b, [(ix, iy), ...] in the order of the walk: both ends, every cell stepped
    into, and at a t == 0 corner both cells that share the corner.  Symmetric in a and b as a set; a == b gives [a]."""
    (x, y), (x1, y1) = (int(a[0]), int(a[1])), (int(b[0]), int(b[1]))
    dx, dy = abs(x1 - x), abs(y1 - y)
    sx, sy = (1 if x1 > x else -1), (1 if y1 > y else -1)
    ix = iy = 0
    out = [(x, y)]
    while ix < dx or iy < dy:
        t = (1 + 2 * ix) * dy - (1 + 2 * iy) * dx
        if t < 0:
            x, ix = x + sx, ix + 1
        elif t > 0:
            y, iy = y + sy, iy + 1
        else:
            out += [(x + sx, y), (x, y + sy)]
            x, y, ix, iy = x + sx, y + sy, ix + 1, iy + 1
        out.append((x, y))
    return out


def grid_team_legs(walk, keep):
    """The legs of a member with the walk c[0 .. A] and the kept indices `keep` -> [(a, b, cells [k][2] int64), ...]: its anchors
    are 0, keep..., A; a leg (a, b) of one action has the cells {c[a], c[b]}, a longer one grid_leg_cells(c[a], c[b])."""
    A = len(walk) - 1
    anchors = [0] + [int(k) for k in keep] + [A]
    legs = []
    for a, b in zip(anchors[:-1], anchors[1:]):
        if b > a:
            legs.append((a, b, np.asarray([walk[a], walk[b]] if b - a == 1 else grid_leg_cells(walk[a], walk[b]), np.int64).reshape(-1, 2)))
    return legs


def grid_leg_layers(walk, keep, layers):
    """Where a member can be, a layer at a time -> a list of T + 1 arrays [k][2] (ix, iy).  With P_t the cells of the leg that
    contains action t (a <= t < b) for t < A and {c[A]} for t >= A: entry t < T is P_t, the tail entry T the union of the P_t with
    t >= min(T, A).  A member without a walk (its start cell alone, keep empty) is in c[0] in every layer."""
    T, A = int(layers), len(walk) - 1
    end = np.asarray([walk[A]], np.int64).reshape(1, 2)
    out = [end] * (T + 1)
    tail = [end]
    for a, b, cells in grid_team_legs(walk, keep):
        for t in range(a, min(b, T)):
            out[t] = cells
        if b > T:
            tail.append(cells)
    out[T] = np.concatenate(tail)
    return out


def grid_reserve_legs(walk, keep, layers, G, reserve):
    """The swept reservation of a smoothed walk, bool [T + 1][G][G]: layer t holds every in-grid cell within Chebyshev distance
    `reserve` of grid_leg_layers(walk, keep, layers)[t] -- a straight leg reserves ALL of itself in EVERY layer of its span, so
    the member may be anywhere on the leg at any time of the span.  When every leg is one action this is grid_reserve(walk, ...)."""
    T, r = int(layers), int(reserve)
    res = np.zeros((T + 1, G, G), bool)
    for t, cells in enumerate(grid_leg_layers(walk, keep, T)):
        for x, y in cells:
            res[t, max(y - r, 0):y + r + 1, max(x - r, 0):x + r + 1] = True
    return res


def grid_team_clearance_legs(walks, keeps, size, layers):
    """The checker of a smoothed team plan, independent of the planner: it sees walks and kept indices only, never maps or fields.
    walks: per robot the cells of its walk; keeps: per robot the kept indices in full, None for a robot WITHOUT a walk (parked:
    UNREACHABLE or UNCONVERGED) -> clearance [n_teams] int32: over every pair of mates that both have a walk, the minimum over all
    layers t <= T of the Chebyshev distance between their sets of grid_leg_layers (the tail layer: the unions); PLAN_NO_PAIR where
    a team has no such pair (size 1).  The guarantee of grid_plan_team(smooth=True) is clearance > reserve: two mates that keep
    to their legs -- leaving no anchor before its release and reaching the next no later than the walk does -- are in cells more
    than `reserve` apart whatever their speeds along the legs."""
    n, size, T = len(walks), int(size), int(layers)
    if size < 1 or n % size != 0 or len(keeps) != n:
        raise ValueError(f"{n} walks and {len(keeps)} lists of kept indices do not split into teams of {size}")
    clear = np.full(n // size, PLAN_NO_PAIR, np.int64)
    sets = [None if keeps[i] is None else grid_leg_layers(walks[i], keeps[i], T) for i in range(n)]
    for i in range(n):
        for j in range(i + 1, (i // size + 1) * size):
            if sets[i] is None or sets[j] is None:
                continue
            for t in range(T + 1):
                p, q = sets[i][t], sets[j][t]
                if t and p is sets[i][t - 1] and q is sets[j][t - 1]:
                    continue                                                  # the same two legs as in the layer before
                clear[i // size] = min(clear[i // size], int(np.abs(p[:, None, :] - q[None, :, :]).max(axis=2).min()))
    return clear.astype(np.int32)


def grid_plan_team(spec, walls, hazards, start, goal, K, teams, reserve, step0=0, layer_steps=None, layers=None, want_fields=True,
                   smooth=False, margin=1, max_leg=8, order=None):
    """The whole team plan of n robots by the rule: grid_plan_time's dict per robot -- there are no shared fields: field_of is the
    identity and fields is int32 [n][T + 1][G][G] (None without want_fields), each robot's own on ITS map -- with occupancy the
    BASE layers bool [S][T + 1][G][G], plus walks (per robot the cells of its walk; a robot without one: its start cell),
    team_clearance and team_crossings [n_teams] int32 (grid_team_clearance).  A member that is UNREACHABLE reserves its start cell
    in every layer: a parked robot is an obstacle, as in team_cost.
    smooth: member m's map is occ_t = base_t OR the earlier members' grid_reserve_legs; grid_team_field and
    grid_walk_team run unchanged on it; nb = grid_next_blocked(los_blocked(occ_t, margin) of every t) is built on that same map, so
    it is the member's own; keep = grid_smooth_time(cells, nb, max_leg) (max_leg None: no cap).  The outputs mean what
    grid_path_smooth_time gives: the waypoints are the centres of the kept cells, then the goal itself; waits all zero; leave[k]
    the action index of waypoint k's anchor; arrive, cost and `moves` as there; release = grid_release_smooth.  The dict gains
    `keeps`, per robot the kept indices in full (not cut at K; [] without a walk).  team_clearance is then
    grid_team_clearance_legs's and the guarantee is team_clearance > reserve: two mates that keep to their legs, leaving no anchor
    before its release and reaching the next no later than the walk does, are in cells more than `reserve` apart whatever their
    speeds; team_crossings stays grid_team_clearance's count on the walks; a later member that has a walk keeps > reserve from an
    earlier parked mate's start cell.  NOT promised: more PLANNED robots than the unsmoothed plan (a long leg reserves all of itself
    for all of its span, hence the cap max_leg); fewer waypoints; anything about a later member's start cell that an earlier
    member's leg covers -- that member comes back UNREACHABLE and is reported as such.
    order: None (the identity) or int [n_teams][size], one permutation of 0 .. size - 1 per team (plan_team_order):
    in team g, position p plans member order[g][p], on the base layers OR the reservations of the members at the positions
    0 .. p - 1.  Every output stays indexed by robot; the plan is grid_plan_team's on the permuted inputs, un-permuted."""
    start, goal = np.asarray(start, np.float32), np.asarray(goal, np.float32)
    n, P = goal.shape
    if layer_steps is None or layers is None:
        raise ValueError("plan_team: layer_steps and layers are required (a team plan is a time plan even in a static scene)")
    step0, layer_steps, T = plan_time_check(step0, layer_steps, layers)
    if smooth:
        if isinstance(margin, bool) or margin not in (0, 1):
            raise ValueError(f"line-of-sight margin must be 0 or 1, got {margin!r}")
        if max_leg is not None:
            max_leg = plan_max_leg_check(max_leg)
    occ, S, scene = plan_team_base(spec, walls, hazards, step0, layer_steps, T)
    for sc in (walls, hazards):
        if sc is not None:
            sc.check_robots(n)
    size, r = plan_team_check(teams, reserve, n, scene)
    G = spec.cells
    one = (T + 1) * G * G * 4
    if one > PLAN_TIME_MAX_BYTES or (want_fields and n * one > PLAN_TIME_MAX_BYTES):
        raise ValueError(f"plan_team: time fields of {n if want_fields else 1} x {T + 1} x {G} x {G} x 4 bytes exceed the cap of "
                         f"{PLAN_TIME_MAX_BYTES} bytes ({PLAN_TIME_MAX_BYTES >> 20} MiB)")
    if smooth and plan_team_smooth_bytes(G, T) > PLAN_TIME_MAX_BYTES:
        raise ValueError(f"plan_team: one team's field, next-blocked table and reservation of {T + 1} x {G} x {G} x 7 bytes exceed the cap "
                         f"of {PLAN_TIME_MAX_BYTES} bytes ({PLAN_TIME_MAX_BYTES >> 20} MiB)")
    gx, gy = spec.cell_of(goal[:, :2])
    sx, sy = spec.cell_of(start[:, :2])
    sc = np.zeros(n, np.int32) if scene is None else np.asarray(scene, np.int32)
    fields = np.zeros((n, T + 1, G, G), np.int32) if want_fields else None
    wp, waits, leave = np.zeros((n, K, P), np.float32), np.zeros((n, K), np.int32), np.zeros((n, K), np.int32)
    count, status, cost, arrive, moves = (np.zeros(n, np.int32) for _ in range(5))
    rows = np.arange(n) if order is None else (np.arange(n) // size * size + plan_team_order(order, n // size, size).ravel())
    walks, keeps = [None] * n, [None] * n
    for j, i in enumerate(rows):
        if j % size == 0:
            res = np.zeros((T + 1, G, G), bool)
        layers_i = occ[sc[i]] | res
        field = grid_team_field(layers_i, int(gy[i]) * G + int(gx[i]))
        if want_fields:
            fields[i] = field
        if smooth:
            (w, count[i], status[i], cost[i], leave[i], arrive[i], moves[i]), cells, keep = grid_path_smooth_team(
                field, layers_i, spec, start[i], goal[i], K, margin, max_leg)
        else:
            (w, count[i], status[i], cost[i], waits[i], leave[i], arrive[i]), cells = grid_path_team(field, layers_i, spec, start[i], goal[i], K)
            keep = list(range(1, len(cells) - 1))
        m = min(int(count[i]), K)
        wp[i, :m, :2] = w[:m]
        wp[i, :m, 2:] = goal[i, 2:]
        walks[i] = cells if cells else [(int(sx[i]), int(sy[i]))]
        keeps[i] = keep
        res |= grid_reserve_legs(walks[i], keep, T, G, r) if smooth else grid_reserve(walks[i], T, G, r)
    first, number = grid_layer_frames(hazards, step0, layer_steps, T) if isinstance(hazards, MovingHazards) else (None, None)
    clear, cross = grid_team_clearance(walks, size, T)
    out = {"waypoints": wp, "n_waypoints": np.minimum(count, K).astype(np.int32), "count": count, "status": status, "cost": cost,
           "waits": waits, "leave": leave, "arrive": arrive,
           "release": grid_release_smooth(leave, step0, layer_steps) if smooth else grid_release(waits, leave, step0, layer_steps),
           "occupancy": occ, "fields": fields, "field_of": np.arange(n, dtype=np.int32),
           "field_goal_cell": (gy * G + gx).astype(np.int32), "field_scene": sc.copy(), "layer_first": first, "layer_number": number,
           "walks": walks, "team_clearance": clear, "team_crossings": cross}
    if smooth:
        out["moves"], out["keeps"] = moves, keeps
        out["team_clearance"] = grid_team_clearance_legs(walks, plan_team_keeps_with_walks(keeps, status), size, T)
    return out


# ---- priority reordering rounds: a team whose plan leaves members parked is planned again with those members first
PLAN_RETRIES_MAX = 8
TEAM_ROUND_KEYS = ("team_order", "team_rounds", "team_parked", "team_parked_first")


def plan_team_order(order, n_teams, size):
    """-> order as int64 [n_teams][size], or ValueError: every row a permutation of 0 .. size - 1"""
    o = np.asarray(order)
    if o.dtype == bool or not np.issubdtype(o.dtype, np.integer) or o.shape != (int(n_teams), int(size)):
        raise ValueError(f"plan_team: order must be integers [n_teams = {int(n_teams)}][size = {int(size)}], got {o.dtype} {o.shape}")
    bad = np.nonzero(np.any(np.sort(o, axis=1) != np.arange(int(size)), axis=1))[0]
    if bad.size:
        raise ValueError(f"plan_team: order of team {int(bad[0])} is not a permutation of 0 .. {int(size) - 1}: {o[bad[0]].tolist()}")
    return o.astype(np.int64)


def plan_retries_check(retries):
    """-> retries as an int, or ValueError: an integer in 0 .. PLAN_RETRIES_MAX (a bool is refused)"""
    if isinstance(retries, bool) or not isinstance(retries, (int, np.integer)) or not 0 <= int(retries) <= PLAN_RETRIES_MAX:
        raise ValueError(f"plan_team: retries must be an integer in 0 .. {PLAN_RETRIES_MAX}, got {retries!r}")
    return int(retries)


def plan_team_parked(status):
    """The members without a walk, bool like status: UNREACHABLE or UNCONVERGED (TRUNCATED has a walk)"""
    status = np.asarray(status)
    return (status == UNREACHABLE) | (status == UNCONVERGED)


def plan_team_next_order(order, parked):
    """The order of the next round, a list: the parked members in their relative order of this round, then the others in theirs.
    order: this round's, [size]; parked: bool [size] indexed by MEMBER"""
    order = [int(m) for m in order]
    return [m for m in order if parked[m]] + [m for m in order if not parked[m]]


def grid_plan_team_rounds(spec, walls, hazards, start, goal, K, teams, reserve, step0=0, layer_steps=None, layers=None, want_fields=True,
                          smooth=False, margin=1, max_leg=8, retries=0):
    """grid_plan_team with up to `retries` (0 .. PLAN_RETRIES_MAX) reordering rounds, every team on its own.  Round 0 plans in the
    identity order.  After round k the team's parked members are those without a walk (plan_team_parked).  Nobody parked: stop.
    Otherwise the next order is plan_team_next_order's -- the parked members first; stop without planning it if k == retries or
    if that order was already planned for this team (which includes: the parked members are in front already).  The result is the
    round with the fewest parked members, the earliest on a tie: the dict is grid_plan_team(order=that round's), bit for bit, plus
    team_order int32 [n_teams][size] (the result's order), team_rounds int32 [n_teams] (rounds planned, >= 1), team_parked and
    team_parked_first int32 [n_teams] (parked members of the result and of round 0).  retries = 0: grid_plan_team's plan.
    What rounds do NOT repair: two mates whose start cells, or whose goal cells, are within `reserve` of each other fail in every
    order (whoever plans second finds its start reserved, or its goal never free); an earlier member still does not know a later
    member's start cell and may plan through it, which parks the later one; and the orders tried are one chain of at most
    retries + 1, not all size! of them -- a team that some order would plan in full may still come back with members parked.
    smooth=True with retries > 0 is refused (ValueError): rounds of smoothed team plans are not built."""
    R_ = plan_retries_check(retries)
    if smooth and R_ > 0:
        raise ValueError("plan_team: retries > 0 with smooth=True is not supported (reordering rounds plan unsmoothed team plans only)")
    kw = dict(step0=step0, layer_steps=layer_steps, layers=layers, want_fields=want_fields, smooth=smooth, margin=margin, max_leg=max_leg)
    out = grid_plan_team(spec, walls, hazards, start, goal, K, teams, reserve, **kw)
    size = teams.size
    g = len(out["status"]) // size
    ident = list(range(size))
    order = np.tile(np.arange(size, dtype=np.int32), (g, 1))                 # the result's
    now = [ident] * g                                                        # the latest round's
    tried = [[ident] for _ in range(g)]
    parked = plan_team_parked(out["status"]).reshape(g, size)
    best = parked.sum(axis=1).astype(np.int32)
    first, rounds = best.copy(), np.ones(g, np.int32)
    live = np.ones(g, bool)
    for k in range(R_ + 1):
        nxt = np.tile(np.arange(size), (g, 1))                               # a team that has stopped: any order, its rows are not used
        for t in np.flatnonzero(live):
            cand = plan_team_next_order(now[t], parked[t])
            if not parked[t].any() or k == R_ or cand in tried[t]:
                live[t] = False
            else:
                nxt[t], now[t] = cand, cand
                tried[t].append(cand)
        if not live.any():
            break
        new = grid_plan_team(spec, walls, hazards, start, goal, K, teams, reserve, order=nxt, **kw)
        status = plan_team_parked(new["status"]).reshape(g, size)
        for t in np.flatnonzero(live):
            rounds[t] += 1
            parked[t] = status[t]
            if status[t].sum() < best[t]:
                best[t], order[t] = status[t].sum(), nxt[t]
                rows = slice(t * size, (t + 1) * size)
                for key in ("waypoints", "n_waypoints", "count", "status", "cost", "waits", "leave", "arrive", "release", "fields"):
                    if out[key] is not None:
                        out[key][rows] = new[key][rows]
                out["walks"][rows] = new["walks"][rows]
                for key in ("team_clearance", "team_crossings"):
                    out[key][t] = new[key][t]
    out.update(team_order=order, team_rounds=rounds, team_parked=best, team_parked_first=first)
    return out


def plan_team_smooth_bytes(G, T):
    """bytes of one team's scratch in a smoothed team plan: the field (4), the next-blocked table (2) and the reservation (1) per
    cell and layer; the engine holds the sum over its workgroups under PLAN_TIME_MAX_BYTES and refuses one that exceeds it"""
    return (int(T) + 1) * int(G) ** 2 * 7


def plan_team_keeps_with_walks(keeps, status):
    """keeps as grid_team_clearance_legs takes them: None for the robots without a walk (UNREACHABLE, UNCONVERGED)"""
    return [None if int(s) in (UNREACHABLE, UNCONVERGED) else list(k) for k, s in zip(keeps, status)]


def grid_path_smooth_team(field, occ_layers, spec, start_xy, goal_xy, K, margin=1, max_leg=8, nb=None):
    """grid_path_smooth_time on grid_walk_team's walk, the legs capped at max_leg actions -> (grid_path_smooth_time's tuple, cells of
    the walk ([] when UNREACHABLE), kept indices in full)"""
    K = int(K)
    if K < 1:
        raise ValueError("max_waypoints must be >= 1")
    wp, leave = np.zeros((K, 2), np.float32), np.zeros(K, np.int32)
    cells, acts, status = grid_walk_team(field, occ_layers, spec, start_xy)
    if status == UNREACHABLE:
        return (wp, 0, UNREACHABLE, -1, leave, 0, 0), [], []
    if nb is None:
        nb = grid_next_blocked([los_blocked(o, margin) for o in np.asarray(occ_layers, bool)])
    keep = grid_smooth_time(cells, nb, max_leg)
    for count, j in enumerate(keep[:K]):
        wp[count] = spec.centre(cells[j][0]), spec.centre(cells[j][1])
    count = len(keep)
    if count < K:
        wp[count] = np.asarray(goal_xy, np.float32)[:2]
    count += 1
    leave[1:min(count, K)] = keep[:min(count, K) - 1]
    sx, sy = cells[0]
    return ((wp, count, TRUNCATED if count > K else PLANNED, int(np.asarray(field)[0, sy, sx]), leave, len(acts),
             sum(k != PLAN_WAIT_ACTION for k in acts)), cells, keep)


# ---- goal assignment inside a team: who takes which goal, a minimum-cost perfect matching per team on each robot's
# own static cost-to-go.  This project's own rule, integers throughout; the device (csrc/kernels_plan.h: k_plan_assign_cost,
# k_plan_assign) is held to it bit for bit, the potentials included.  It runs in front of a team plan and changes the plan's INPUT
# (goal[n]), never the planner; reservations play no part, so the matching is a function of (scene, starts, goals) alone.
PLAN_ASSIGN_NONE = 1 << 21      # the cost of a pair without a path: above 16 * 7 * 128 * 128, the largest total of real costs
PLAN_ASSIGN_FORBID = 1 << 26    # in a makespan matching: the cost of a pair above the bottleneck L
PLAN_ASSIGN_OBJECTIVES = ("sum", "makespan")
ASSIGN_KEYS = ("assign", "goal", "assign_cost", "assign_total", "assign_max", "assign_identity_total", "assign_identity_max",
               "assign_changed", "assign_status")


def plan_assign_objective(objective):
    """-> the index of `objective` in PLAN_ASSIGN_OBJECTIVES, or ValueError"""
    if not isinstance(objective, str) or objective not in PLAN_ASSIGN_OBJECTIVES:
        raise ValueError(f"plan_assign: objective must be one of {PLAN_ASSIGN_OBJECTIVES}, got {objective!r}")
    return PLAN_ASSIGN_OBJECTIVES.index(objective)


def plan_assign_match(C):
    """The minimum-total perfect matching of the square int64 matrix C (row i takes column col_of_row[i]) by the shortest-augmenting-
    path Hungarian method with row and column potentials -> (col_of_row [n] int64, u [n] int64, v [n] int64).  THIS TEXT IS THE
    DEFINITION, ties included: rows are inserted in index order; every scan relaxes the unused columns from the row i0 that was
    reached last (minv[j] = min(minv[j], C[i0][j] - u[i0] - v[j]), strict <, so the earlier way is kept on a tie) and takes the unused
    column of least minv, the lowest index on a tie (strict <); delta goes onto u of the rows in the tree and off v of the used
    columns and off minv of the others.  On return u[i] + v[j] <= C[i][j] everywhere, with equality on the matched pairs -- the
    certificate that the total is the least one (any matching's total is >= sum(u) + sum(v))."""
    C = np.asarray(C, np.int64)
    n = C.shape[0]
    if C.ndim != 2 or C.shape[1] != n:
        raise ValueError(f"plan_assign: the cost matrix must be square, got shape {C.shape}")
    big = np.int64(1) << 62
    u, v = np.zeros(n, np.int64), np.zeros(n, np.int64)
    p = np.full(n, -1, np.int64)                       # p[j]: the row matched to column j
    for i in range(n):
        minv, way = np.full(n, big, np.int64), np.full(n, -1, np.int64)   # way[j]: the column before j on its path, -1: the root
        used, rowin = np.zeros(n, bool), np.zeros(n, bool)
        j0, i0 = -1, i
        while True:
            rowin[i0] = True
            open_ = ~used
            cur = C[i0] - u[i0] - v
            better = open_ & (cur < minv)
            minv[better], way[better] = cur[better], j0
            j1 = int(np.argmin(np.where(open_, minv, big)))                # argmin: the first of equal values
            delta = minv[j1]
            u[rowin] += delta
            v[used] -= delta
            minv[open_] -= delta
            j0 = j1
            used[j0] = True
            i0 = int(p[j0])
            if i0 < 0:
                break
        while j0 >= 0:                                                     # augment along the way back to the root
            j1 = int(way[j0])
            p[j0] = p[j1] if j1 >= 0 else i
            j0 = j1
    col = np.zeros(n, np.int64)
    col[p] = np.arange(n)
    return col, u, v


def plan_assign_bottleneck(C):
    """L: the least value such that a perfect matching exists among the entries of C that are <= L (unique, so any method serves):
    a bisection over the sorted distinct entries; a value is feasible where the 0 / 1 matrix C > L has a matching of total 0"""
    C = np.asarray(C, np.int64)
    cand = np.unique(C)
    lo, hi = 0, len(cand) - 1                                              # the largest entry is feasible
    while lo < hi:
        mid = (lo + hi) // 2
        B = (C > cand[mid]).astype(np.int64)
        col, _, _ = plan_assign_match(B)
        if int(B[np.arange(len(col)), col].sum()) == 0:
            hi = mid
        else:
            lo = mid + 1
    return int(cand[lo])


def plan_assign_team(C, objective="sum"):
    """One team's assignment on its int64 cost matrix C (NONE entries as PLAN_ASSIGN_NONE) -> (col_of_row, u, v, changed).
    "sum": plan_assign_match(C).  "makespan": plan_assign_match on where(C > L, PLAN_ASSIGN_FORBID, C), L = plan_assign_bottleneck(C):
    the largest member cost first, then the total.  Identity first: where the identity's total (makespan: its (max, total)) on C
    equals the matching's, the identity is the result -- a team that is well paired already is never renumbered.  u, v: the
    potentials of the (last) plan_assign_match run, whichever matching is returned (the identity is then optimal too, hence tight)."""
    C = np.asarray(C, np.int64)
    n = C.shape[0]
    rows = np.arange(n)
    if plan_assign_objective(objective) == 1:
        L = plan_assign_bottleneck(C)
        col, u, v = plan_assign_match(np.where(C > L, np.int64(PLAN_ASSIGN_FORBID), C))
        same = int(C[rows, rows].max()) == int(C[rows, col].max()) and int(C[rows, rows].sum()) == int(C[rows, col].sum())
    else:
        col, u, v = plan_assign_match(C)
        same = int(C[rows, rows].sum()) == int(C[rows, col].sum())
    if same:
        col = rows.astype(np.int64)
    return col, u, v, bool(np.any(col != rows))


def plan_assign_cells(spec, start, goal):
    """-> (start cell [n], goal cell [n]) int64 flat indices of float32 starts and goals [n][>= 2]"""
    sx, sy = spec.cell_of(np.asarray(start, np.float32)[:, :2])
    gx, gy = spec.cell_of(np.asarray(goal, np.float32)[:, :2])
    return sy * spec.cells + sx, gy * spec.cells + gx


def plan_assign_check(spec, walls, hazards, start, goal, teams, objective, step0, layer_steps, layers):
    """grid_assign's refusals, by name -> (start, goal float32 [n][P], size, objective index, step0, layer_steps, T); T = 0 (and
    layer_steps = 1) in a static scene, where neither is looked at"""
    if not isinstance(spec, GridSpec):
        raise TypeError(f"spec must be a mobrob_amd.envs.goal_rules.GridSpec, not {type(spec).__name__}")
    if not isinstance(teams, Teams):
        raise TypeError(f"plan_assign: teams must be a mobrob_amd.envs.goal_rules.Teams, not {type(teams).__name__}")
    obj = plan_assign_objective(objective)
    start, goal = np.asarray(start, np.float64), np.asarray(goal, np.float64)
    if goal.ndim != 2 or goal.shape[0] < 1 or goal.shape[1] not in (2, 3) or start.shape != goal.shape:
        raise ValueError(f"plan_assign: start and goal must both be [n_robots, 2 or 3], got shapes {start.shape} and {goal.shape}")
    if not (np.all(np.isfinite(start)) and np.all(np.isfinite(goal))):
        raise ValueError("plan_assign: start and goal must be finite")
    if isinstance(hazards, MovingHazards):
        if layer_steps is None or layers is None:
            raise ValueError("plan_assign: layer_steps and layers are required with a MovingHazards (the cost map is the tail of its layers)")
        step0, layer_steps, T = plan_time_check(step0, layer_steps, layers)
        _, scene = plan_scene_time(walls, hazards)
    else:
        step0, layer_steps, T = 0, 1, 0
        _, scene = plan_scene(walls, hazards)
    n = goal.shape[0]
    for sc in (walls, hazards):
        if sc is not None:
            sc.check_robots(n)
    size, _ = plan_team_check(teams, 0, n, scene)
    return start.astype(np.float32), goal.astype(np.float32), size, obj, step0, layer_steps, T


def plan_assign_outputs(C, col, changed, goal, status=None):
    """The outputs of an assignment from the cost matrices C int64 [n_teams][size][size] (NONE as PLAN_ASSIGN_NONE), the matchings
    col [n_teams][size] and goal float32 [n][P] -> grid_assign's dict without the matrix and the potentials"""
    g, size = C.shape[:2]
    rows = np.arange(size)
    base = (np.arange(g) * size)[:, None]
    assign = (base + col).reshape(-1).astype(np.int32)
    picked, ident = C[np.arange(g)[:, None], rows[None, :], col], C[:, rows, rows]
    return {"assign": assign, "goal": np.asarray(goal, np.float32)[assign],
            "assign_cost": np.where(picked >= PLAN_ASSIGN_NONE, -1, picked).reshape(-1).astype(np.int32),
            "assign_total": picked.sum(axis=1).astype(np.int64), "assign_max": picked.max(axis=1).astype(np.int32),
            "assign_identity_total": ident.sum(axis=1).astype(np.int64), "assign_identity_max": ident.max(axis=1).astype(np.int32),
            "assign_changed": np.asarray(changed, bool),
            "assign_status": np.full(g, PLANNED, np.int32) if status is None else np.asarray(status, np.int32)}


def grid_assign(spec, walls, hazards, start, goal, teams, objective="sum", step0=0, layer_steps=None, layers=None, want_matrix=True):
    """Who takes which goal inside every team -> dict.  The cost map is layer T of the team plan's base layers
    (plan_team_base): grid_occupancy's map in a static scene, the conservative tail of grid_occupancy_time with a MovingHazards
    (layer_steps and layers are required only then).  Per team g the int64 matrix C[g][i][j] = grid_field(map of the team's scene,
    goal cell of member j)[start cell of member i], -1 (blocked or unreachable) as PLAN_ASSIGN_NONE -- so a minimum-sum matching
    first minimises the number of pairs without a path -- and plan_assign_team(C[g], objective) is the team's matching; a team of
    one keeps the identity.  The dict: assign int32 [n] (the robot, a mate or itself, whose INPUT goal robot i is given), goal
    float32 [n][P] = goal[assign], assign_cost int32 [n] (-1: no path), assign_total int64 and assign_max int32 [n_teams] (on C, NONE
    counted as NONE), assign_identity_total and assign_identity_max (the same of the pairing as given), assign_changed bool
    [n_teams], assign_status int32 [n_teams] (PLANNED; the device reports UNCONVERGED where a field hit its sweep bound, and that
    team keeps the identity), assign_potentials (u, v) int64 [n_teams][size] each (plan_assign_match's certificate, of the last
    run), and with want_matrix assign_matrix int32 [n_teams][size][size], -1 for NONE."""
    start, goal, size, _, step0, layer_steps, T = plan_assign_check(spec, walls, hazards, start, goal, teams, objective, step0,
                                                                     layer_steps, layers)
    occ, _, scene = plan_team_base(spec, walls, hazards, step0, layer_steps, T)
    cost_map = occ[:, T]
    n = goal.shape[0]
    g = n // size
    sc = np.zeros(n, np.int64) if scene is None else np.asarray(scene, np.int64)
    scell, gcell = plan_assign_cells(spec, start, goal)
    fields = {}
    C = np.zeros((g, size, size), np.int64)
    for t in range(g):
        for j in range(size):
            nj = t * size + j
            key = (int(sc[nj]), int(gcell[nj]))
            if key not in fields:
                fields[key] = grid_field(cost_map[key[0]], key[1]).reshape(-1)
            d = fields[key][scell[t * size:(t + 1) * size]].astype(np.int64)
            C[t, :, j] = np.where(d < 0, PLAN_ASSIGN_NONE, d)
    col, u, v = np.zeros((g, size), np.int64), np.zeros((g, size), np.int64), np.zeros((g, size), np.int64)
    changed = np.zeros(g, bool)
    for t in range(g):
        col[t], u[t], v[t], changed[t] = plan_assign_team(C[t], objective)
    out = plan_assign_outputs(C, col, changed, goal)
    out["assign_potentials"] = (u, v)
    if want_matrix:
        out["assign_matrix"] = np.where(C >= PLAN_ASSIGN_NONE, -1, C).astype(np.int32)
    return out


# ---- run specifications: reach / avoid / until robustness per robot, from the positions of a run (the device: csrc/kernels_spec.h,
# k_spec_monitor, csrc/kernels_spec_nested.h, k_spec_monitor_nested, for a specification with a nested clause, and
# csrc/kernels_spec_moving.h, k_spec_monitor_moving, for one with moving regions or a mate predicate; all held to this bit for bit).
# Stated here once; waypoints.monitor, the host loop and PPOEngine.spec_monitor apply it.
SPEC_REGIONS_MAX = 64           # regions per scene
SPEC_CLAUSES_MAX = 16           # clauses of a specification
SPEC_OPEN = 2 ** 31 - 1         # the right end of an open window
SPEC_ALWAYS, SPEC_EVENTUALLY, SPEC_UNTIL = 0, 1, 2
SPEC_STAY, SPEC_RECUR = 3, 4    # the nested clauses: eventually-always and always-eventually over a sliding window (spec_fold)
SPEC_HOLD_MAX = 255             # the longest inner window [t, t + h] of a nested clause
SPEC_WINDOW_SLOTS = 512         # the sum of (h + 1) over the nested clauses of a specification (the device's window block)
SPEC_BOX, SPEC_CIRCLE = 0, 1    # region kinds
SPEC_RESULT_KEYS = ("spec_rho", "spec_witness", "robustness", "weakest", "satisfied")
SPEC_FRAMES_MAX_BYTES = 64 << 20   # cap on a MovingRegions table (S * F * R * 16 bytes); the engine refuses a larger one too
SPEC_PRED_REGIONS, SPEC_PRED_TOGETHER, SPEC_PRED_APART = 0, 1, 2   # what a predicate reads: a region range, or the team-mates


class Regions:
    """The regions a specification speaks about: `rows` [R, 4] (one scene) or [S, R, 4] (scenes) float32, `kinds` [R] or [S, R]:
    kind 0 (SPEC_BOX) an axis-aligned box (cx, cy, hx, hy) with hx, hy >= 0, kind 1 (SPEC_CIRCLE) a circle (cx, cy, r, 0) with
    r >= 0; `counts` [S] regions in use per scene (None: all R), `scene` [n] scene of each robot (None: S must be 1).  R <=
    SPEC_REGIONS_MAX.  Only x and y count, as for hazards and walls, for drones too.  Checked on construction (ValueError)."""

    def __init__(self, rows, kinds, counts=None, scene=None):
        rw = np.asarray(rows, np.float64)
        if rw.size == 0 and rw.ndim < 2:
            rw = rw.reshape(0, 4)
        if rw.ndim == 2:
            rw = rw[None]
        if rw.ndim != 3 or rw.shape[2] != 4:
            raise ValueError(f"region rows must be [R, 4] or [S, R, 4], got shape {np.shape(rows)}")
        S, R = rw.shape[:2]
        if S < 1:
            raise ValueError("regions need at least one scene")
        if R > SPEC_REGIONS_MAX:
            raise ValueError(f"at most {SPEC_REGIONS_MAX} regions per scene, got {R}")
        kd = np.asarray(kinds)
        if kd.size == 0:
            kd = np.zeros((S, R), np.int32)
        if kd.shape == (R,):
            kd = np.broadcast_to(kd, (S, R))
        if kd.shape != (S, R) or not np.issubdtype(kd.dtype, np.integer):
            raise ValueError(f"region kinds must be [{R}] or [{S}, {R}] integers, got {kd.dtype} of shape {kd.shape}")
        if np.any((kd != SPEC_BOX) & (kd != SPEC_CIRCLE)):
            raise ValueError("region kinds must be 0 (box) or 1 (circle)")
        if not np.all(np.isfinite(rw)) or np.any(np.abs(rw) > np.finfo(np.float32).max):
            raise ValueError("region rows must be finite")
        if np.any(rw[..., 2] < 0) or np.any((kd == SPEC_BOX) & (rw[..., 3] < 0)):
            raise ValueError("box half extents and circle radii must be >= 0")
        if counts is None:
            cnt = np.full(S, R, np.int32)
        else:
            cnt = np.asarray(counts)
            if cnt.shape != (S,) or not np.issubdtype(cnt.dtype, np.integer) or np.any(cnt < 0) or np.any(cnt > R):
                raise ValueError(f"region counts must be {S} integers in 0 .. {R}")
            cnt = cnt.astype(np.int32)
        if scene is None:
            if S != 1:
                raise ValueError(f"{S} region scenes need a scene index per robot")
            sc = None
        else:
            sc = np.asarray(scene)
            if sc.ndim != 1 or not np.issubdtype(sc.dtype, np.integer) or np.any(sc < 0) or np.any(sc >= S):
                raise ValueError(f"region scene indices must be integers in 0 .. {S - 1}")
            sc = np.ascontiguousarray(sc, np.int32)
        self.table = np.ascontiguousarray(rw, np.float32)     # [S, R, 4]
        self.kinds = np.ascontiguousarray(kd, np.int32)       # [S, R]
        self.counts, self.scene = cnt, sc

    @property
    def n_scenes(self):
        return self.table.shape[0]

    @property
    def max_regions(self):
        return self.table.shape[1]

    def check_robots(self, n):
        if self.scene is not None and self.scene.shape != (n,):
            raise ValueError(f"region scene must have {n} entries, one per robot, got {self.scene.shape[0]}")

    @staticmethod
    def from_walls(walls):
        """Every wall as a box region: the box itself, not inflated by the robot radius; scenes and counts are the walls' own."""
        return Regions(walls.table, np.full(walls.table.shape[:2], SPEC_BOX, np.int32), walls.counts, walls.scene)

    @staticmethod
    def from_hazards(hazards):
        """Every hazard as a circle region of its radius; scenes and counts are the hazards' own."""
        t = hazards.table
        rows = np.concatenate([t, np.zeros(t.shape[:2] + (1,), np.float32)], axis=-1)
        return Regions(rows, np.full(t.shape[:2], SPEC_CIRCLE, np.int32), hazards.counts, hazards.scene)


class MovingRegions:
    """Regions that move: `Regions` plus a time axis of F piecewise-constant FRAMES, as MovingHazards is to Hazards.  `rows`
    [F, R, 4] (one scene) or [S, F, R, 4], stored as float32 [S, F, R, 4]; `kinds` [R] or [S, R] -- a region keeps its kind over
    the frames --; `frame_steps` >= 1 steps per frame; `loop`: wrap around after the last frame instead of holding it; `counts`
    and `scene` as for `Regions`.  R <= SPEC_REGIONS_MAX, F >= 1, and the table holds at most SPEC_FRAMES_MAX_BYTES.  Every check
    of `Regions` applies per frame.  Checked on construction (ValueError).

    Time: the sample at tau reads the frame f(max(tau - 1, 0)) with f MovingHazards.frame_index's rule.  A sample at tau >= 1 is
    the position after the step with 0-based global number tau - 1, whose hazard check uses f(tau - 1): a clause over hazards
    sees the frame the run's own hazard check saw.  Nothing is interpolated."""

    def __init__(self, rows, kinds, frame_steps=1, loop=False, counts=None, scene=None):
        rw = np.asarray(rows, np.float64)
        if rw.ndim == 3:
            rw = rw[None]
        if rw.ndim != 4 or rw.shape[3] != 4:
            raise ValueError(f"moving region rows must be [F, R, 4] or [S, F, R, 4], got shape {np.shape(rows)}")
        S, F, R = rw.shape[:3]
        if S < 1:
            raise ValueError("regions need at least one scene")
        if F < 1:
            raise ValueError("moving regions need at least one frame")
        if R > SPEC_REGIONS_MAX:
            raise ValueError(f"at most {SPEC_REGIONS_MAX} regions per scene, got {R}")
        if S * F * R * 16 > SPEC_FRAMES_MAX_BYTES:
            raise ValueError(f"region frames of {S} x {F} x {R} x 16 bytes exceed the cap of {SPEC_FRAMES_MAX_BYTES} bytes "
                             f"({SPEC_FRAMES_MAX_BYTES >> 20} MiB)")
        if isinstance(frame_steps, bool) or not isinstance(frame_steps, (int, np.integer)) or frame_steps < 1:
            raise ValueError(f"frame_steps must be an integer >= 1, got {frame_steps!r}")
        if frame_steps > 2 ** 31 - 1:
            raise ValueError("frame_steps must fit an int32")
        first = Regions(rw[:, 0], kinds, counts, scene)   # kinds, counts, scene and frame 0: Regions' checks
        kd = first.kinds
        if not np.all(np.isfinite(rw)) or np.any(np.abs(rw) > np.finfo(np.float32).max):
            raise ValueError("region rows must be finite")
        if np.any(rw[..., 2] < 0) or np.any((kd[:, None, :] == SPEC_BOX) & (rw[..., 3] < 0)):
            raise ValueError("box half extents and circle radii must be >= 0")
        self.table = np.ascontiguousarray(rw, np.float32)     # [S, F, R, 4]
        self.kinds, self.counts, self.scene = kd, first.counts, first.scene
        self.frame_steps, self.loop = int(frame_steps), bool(loop)

    @property
    def n_scenes(self):
        return self.table.shape[0]

    @property
    def n_frames(self):
        return self.table.shape[1]

    @property
    def max_regions(self):
        return self.table.shape[2]

    check_robots = Regions.check_robots
    frame_index = MovingHazards.frame_index

    def frame_at(self, tau):
        """The frame in force at the sample tau: frame_index(max(tau - 1, 0))."""
        return self.frame_index(max(int(tau) - 1, 0))

    @staticmethod
    def from_hazards(moving_hazards):
        """Every hazard as a circle region of its per-frame radius; scenes, counts, frame_steps and loop are the hazards' own."""
        if not isinstance(moving_hazards, MovingHazards):
            raise TypeError(f"MovingRegions.from_hazards takes a MovingHazards, not {type(moving_hazards).__name__}")
        t = moving_hazards.table
        rows = np.concatenate([t, np.zeros(t.shape[:3] + (1,), np.float32)], axis=-1)
        return MovingRegions(rows, np.full((t.shape[0], t.shape[2]), SPEC_CIRCLE, np.int32), moving_hazards.frame_steps,
                             moving_hazards.loop, moving_hazards.counts, moving_hazards.scene)

    @staticmethod
    def join(static_regions, moving):
        """The static regions first (indices 0 .. Rs - 1, equal in every frame), then the moving ones (Rs .. Rs + Rm - 1); frames,
        frame_steps and loop are `moving`'s.  The scenes and scene indices of both must agree, and every static count must equal
        Rs: `counts` names a prefix of a scene's regions, and a static scene that uses fewer than Rs would put unused rows before
        the moving ones."""
        if not isinstance(static_regions, Regions) or not isinstance(moving, MovingRegions):
            raise TypeError("MovingRegions.join takes (a Regions, a MovingRegions)")
        Rs, F = static_regions.max_regions, moving.n_frames
        if static_regions.n_scenes != moving.n_scenes:
            raise ValueError(f"join: the static regions have {static_regions.n_scenes} scenes, the moving ones {moving.n_scenes}")
        if (static_regions.scene is None) != (moving.scene is None) or (
                moving.scene is not None and not np.array_equal(static_regions.scene, moving.scene)):
            raise ValueError("join: the static and the moving regions must have the same scene index per robot")
        if np.any(static_regions.counts != Rs):
            raise ValueError(f"join: static counts must all equal the {Rs} static regions (counts name a prefix of a scene's regions), "
                             f"got {static_regions.counts.tolist()}")
        rows = np.concatenate([np.broadcast_to(static_regions.table[:, None], (moving.n_scenes, F, Rs, 4)), moving.table], axis=2)
        return MovingRegions(rows, np.concatenate([static_regions.kinds, moving.kinds], axis=1), moving.frame_steps, moving.loop,
                             moving.counts + Rs, moving.scene)


def region_margins(xy, rows, kinds):
    """The INSIDE margin of every region at every position: xy [n, 2], rows [n, R, 4], kinds [n, R] -> [n, R] float32.  float32,
    every operation rounded on its own, no fma.  Box: m = -sdf with sdf exactly as wall_check states it (the device: wall_sdf of
    csrc/kernels_wall.h).  Circle: m = r - sqrt(dx * dx + dy * dy) with dx = px - cx, each product, the sum and the root rounded
    (the device: the distance of csrc/kernels_hazard.h).  Positive inside, 0 (-0.0 for a box) on the boundary, negative outside."""
    f32 = np.float32
    xy, rows = np.asarray(xy, f32), np.asarray(rows, f32)
    px, py = xy[:, None, 0], xy[:, None, 1]
    cx, cy, e2, e3 = (rows[..., j] for j in range(4))
    zero = f32(0)
    with np.errstate(over="ignore", invalid="ignore"):
        dx, dy = px - cx, py - cy
        qx, qy = np.abs(dx) - e2, np.abs(dy) - e3
        ox, oy = np.maximum(qx, zero), np.maximum(qy, zero)
        sdf = np.sqrt(ox * ox + oy * oy) + np.minimum(np.maximum(qx, qy), zero)
        circle = e2 - np.sqrt(dx * dx + dy * dy)
    return np.where(np.asarray(kinds) == SPEC_CIRCLE, circle, -sdf).astype(f32)


def inside(lo, hi=None):
    """The predicate "inside the union of the regions lo .. hi - 1" (hi=None: the single region lo): its value is the largest
    inside margin of the range."""
    return _predicate(lo, hi, False)


def outside(lo, hi=None):
    """The predicate "outside every region lo .. hi - 1" (hi=None: the single region lo): minus the largest inside margin."""
    return _predicate(lo, hi, True)


def _predicate(lo, hi, out):
    lo = int(lo)
    hi = lo + 1 if hi is None else int(hi)
    if lo < 0 or hi < lo:
        raise ValueError(f"a predicate's region range must obey 0 <= lo <= hi, got [{lo}, {hi})")
    return (lo, hi, bool(out))


def together(d):
    """The mate predicate "every team-mate is within d": the minimum over the mates of d - distance (+inf in a team of one)."""
    return _mate_predicate(SPEC_PRED_TOGETHER, d)


def apart(d):
    """The mate predicate "every team-mate is further than d": minus the maximum over the mates of d - distance (+inf in a team
    of one)."""
    return _mate_predicate(SPEC_PRED_APART, d)


def _mate_predicate(kind, d):
    d = float(d)
    if not np.isfinite(d) or d < 0 or d > float(np.finfo(np.float32).max):
        raise ValueError(f"a mate predicate's distance must be finite and >= 0, got {d}")
    return ("mates", kind, float(np.float32(d)))   # the float32 value every path uses


def _is_region_predicate(p):
    return isinstance(p, tuple) and len(p) == 3 and p[0] != "mates"


def _is_mate_predicate(p):
    return isinstance(p, tuple) and len(p) == 3 and p[0] == "mates" and p[1] in (SPEC_PRED_TOGETHER, SPEC_PRED_APART)


def spec_predicate_words(pred):
    """A predicate as the C ABI takes it: (lo, hi, out, kind, radius); a mate predicate has the empty range [0, 0)."""
    if _is_mate_predicate(pred):
        return 0, 0, 0, pred[1], pred[2]
    return pred[0], pred[1], int(pred[2]), SPEC_PRED_REGIONS, 0.0


class Spec:
    """A specification: the conjunction of at most SPEC_CLAUSES_MAX clauses over `regions` (a Regions or a MovingRegions).  A
    clause is built by Spec.always(pred, a, b), Spec.eventually(pred, a, b) or Spec.until(pred1, pred2, a, b) with predicates from
    inside() / outside() / together() / apart() and a window [a, b] in sample time tau -- the number of global steps completed, tau = 0 the start of the run --,
    0 <= a <= b, b=None open (SPEC_OPEN).  See spec_fold for the meaning.

    The two nested clauses fold a sliding-window extremum of their predicate:
      Spec.stay(pred, hold, a, b)     eventually_[a,b] always_[0,hold] pred: inside for hold + 1 consecutive samples, somewhere
      Spec.recur(pred, every, a, b)   always_[a,b] eventually_[0,every] pred: in every window of every + 1 samples at least once
    with h = hold (or every) an integer in 0 .. SPEC_HOLD_MAX and [a, b] bounding the START t of the inner window [t, t + h].  The
    sum of (h + 1) over a specification's nested clauses is at most SPEC_WINDOW_SLOTS.  A window that the run ends before
    completing is not folded: a stay whose hold outlasts the run reads -inf, a recur with no complete window +inf (as an ALWAYS
    whose window never opened).  h = 0 is eventually / always, bit for bit, witness included.  "Stay until the end of the run" is
    no operator of its own: on a finite trace of T steps it is the last sample, and stay(pred, hold, a=T - hold, b=T - hold) asks
    for the last hold + 1 samples.

    Things that move.  `regions` may be a MovingRegions: the sample at tau reads the frame MovingRegions.frame_at(tau), the one
    the run's own hazard check saw.  The mate predicates together(d) / apart(d) speak about the robot's team: `team_size` (one of
    TEAM_SIZES) consecutive robots, robot i with the mates j = (i // size) * size + m, m ascending, j != i, each at the position
    this sample's record holds for it (an idle mate stands where its row says).  g_j = d - dist_ij with the circle margin's
    arithmetic, the mate as the centre; together(d) is the minimum of the g_j by explicit <, from +inf; apart(d) minus their
    maximum by explicit >, from -inf; a team of one reads +inf for both.  They stand wherever inside / outside do, in all five
    clause kinds.  `dynamic` is True for a specification with moving regions or a mate predicate (the device folds it with
    k_spec_monitor_moving); one without either is the object it was and takes the call it took.

    A specification can also drive the plan: spec_plan (GridPlanner.plan_spec) turns the always(outside) clauses over the whole run
    into obstacles and the eventually / stay clauses over inside() into stations, and chooses their order per robot.

    Not built: deeper nesting (an until inside a window, a window inside a window), disjunction of clauses, predicates on
    velocity, interpolation between frames; in a plan from a specification: until, recur, mate predicates and moving regions."""

    def __init__(self, regions, clauses, team_size=1):
        if not isinstance(regions, (Regions, MovingRegions)):
            raise TypeError(f"regions must be a mobrob_amd.envs.goal_rules.Regions, not {type(regions).__name__}")
        if isinstance(team_size, bool) or not isinstance(team_size, (int, np.integer)) or int(team_size) not in TEAM_SIZES:
            raise ValueError(f"a specification's team_size must be one of {TEAM_SIZES}, got {team_size!r}")
        clauses = list(clauses)
        if not 1 <= len(clauses) <= SPEC_CLAUSES_MAX:
            raise ValueError(f"a specification has 1 .. {SPEC_CLAUSES_MAX} clauses, got {len(clauses)}")
        R = regions.max_regions
        for c, cl in enumerate(clauses):
            flat = isinstance(cl, tuple) and len(cl) == 5 and cl[0] in (SPEC_ALWAYS, SPEC_EVENTUALLY, SPEC_UNTIL)
            nested = isinstance(cl, tuple) and len(cl) == 6 and cl[0] in (SPEC_STAY, SPEC_RECUR)
            if not (flat or nested):
                raise TypeError(f"clause {c} is not one of Spec.always / Spec.eventually / Spec.until / Spec.stay / Spec.recur")
            for p in cl[3:5]:
                if not (_is_region_predicate(p) or _is_mate_predicate(p)):
                    raise TypeError(f"clause {c}: a predicate comes from inside() / outside() / together() / apart()")
                if _is_region_predicate(p) and p[1] > R:
                    raise ValueError(f"clause {c}: region range [{p[0]}, {p[1]}) outside 0 .. {R}")
            if nested:
                _hold(cl[5], f"clause {c}: hold")
        self.regions, self.clauses, self.team_size = regions, tuple(clauses), int(team_size)
        self.moving = isinstance(regions, MovingRegions)
        self.mates = any(_is_mate_predicate(p) for cl in self.clauses for p in cl[3:5])
        self.dynamic = self.moving or self.mates
        # per clause: the inner window's h (0 for a flat clause) and where its h values start in SpecState.tail
        self.holds = tuple(cl[5] if len(cl) == 6 else 0 for cl in self.clauses)
        self.nested = any(len(cl) == 6 for cl in self.clauses)
        self.tail_offsets = tuple(int(v) for v in np.cumsum((0,) + self.holds)[:-1])
        self.tail_width = sum(self.holds)
        slots = sum(h + 1 for cl, h in zip(self.clauses, self.holds) if len(cl) == 6)
        if slots > SPEC_WINDOW_SLOTS:
            raise ValueError(f"the nested clauses' windows take {slots} slots (the sum of hold + 1), above SPEC_WINDOW_SLOTS = "
                             f"{SPEC_WINDOW_SLOTS}")

    @property
    def n_clauses(self):
        return len(self.clauses)

    def check_robots(self, n):
        """The regions' check of the robot count, and the teams': n must split into teams of team_size."""
        self.regions.check_robots(n)
        if int(n) % self.team_size != 0:
            raise ValueError(f"{int(n)} robots do not split into the specification's teams of {self.team_size}")

    @staticmethod
    def _clause(op, pred1, pred2, a, b):
        a = int(a)
        b = SPEC_OPEN if b is None else int(b)
        if not 0 <= a <= b <= SPEC_OPEN:
            raise ValueError(f"a window must obey 0 <= a <= b, got [{a}, {b}]")
        for p in (pred1, pred2):
            if not (isinstance(p, tuple) and len(p) == 3):
                raise TypeError("a predicate comes from inside() or outside(), together() or apart()")
        return (op, a, b, pred1, pred2)

    @staticmethod
    def always(pred, a=0, b=None):
        return Spec._clause(SPEC_ALWAYS, pred, pred, a, b)

    @staticmethod
    def eventually(pred, a=0, b=None):
        return Spec._clause(SPEC_EVENTUALLY, pred, pred, a, b)

    @staticmethod
    def until(pred1, pred2, a=0, b=None):
        return Spec._clause(SPEC_UNTIL, pred1, pred2, a, b)

    @staticmethod
    def stay(pred, hold, a=0, b=None):
        """eventually_[a,b] always_[0,hold] pred: the best, over the window starts t in [a, b], of the worst value in [t, t + hold]"""
        return Spec._clause(SPEC_STAY, pred, pred, a, b) + (_hold(hold, "stay: hold"),)

    @staticmethod
    def recur(pred, every, a=0, b=None):
        """always_[a,b] eventually_[0,every] pred: the worst, over the window starts t in [a, b], of the best value in [t, t + every]"""
        return Spec._clause(SPEC_RECUR, pred, pred, a, b) + (_hold(every, "recur: every"),)


def _hold(h, what):
    if isinstance(h, bool) or not isinstance(h, (int, np.integer)) or not 0 <= h <= SPEC_HOLD_MAX:
        raise ValueError(f"{what} must be an integer in 0 .. SPEC_HOLD_MAX = {SPEC_HOLD_MAX}, got {h!r}")
    return int(h)


def spec_key(v):
    """The total order on float32 bits as an int32 key: key = i ^ ((i >> 31) & 0x7fffffff) on the int32 view, so that -0.0 < +0.0
    and every bit pattern has its place.  The inner extremum of a nested clause is taken under it: a box margin is -0.0 on the
    boundary and a circle's +0.0, and under float comparison the bits of a window's minimum would depend on the order in which an
    implementation visits the window.  With the key a ring rescan, a monotonic queue and a block scan all give the same bits."""
    i = np.ascontiguousarray(v, np.float32).view(np.int32)
    return i ^ ((i >> 31) & np.int32(0x7fffffff))


class SpecState:
    """What a specification carries per robot from call to call of a run: val [n][C][2] float32 (rho, guard), wit [n][C] int32
    (the witness sample, -1 = none) and tail [n][W] float32, W the sum of h over the nested clauses in clause order: for each
    nested clause the last h values of its predicate, oldest first (chronological, not a ring position, so that two
    implementations agree on its bits).  tail=None is [n][0], the tail of a specification without nested clauses."""

    def __init__(self, val, wit, tail=None):
        self.val, self.wit = np.ascontiguousarray(val, np.float32), np.ascontiguousarray(wit, np.int32)
        if self.val.ndim != 3 or self.val.shape[2] != 2 or self.wit.shape != self.val.shape[:2]:
            raise ValueError(f"a SpecState is val [n][C][2] and wit [n][C], got {self.val.shape} and {self.wit.shape}")
        self.tail = np.zeros((self.val.shape[0], 0), np.float32) if tail is None else np.ascontiguousarray(tail, np.float32)
        if self.tail.ndim != 2 or self.tail.shape[0] != self.val.shape[0]:
            raise ValueError(f"a SpecState's tail is [n][W] with n = {self.val.shape[0]}, got {self.tail.shape}")

    def copy(self):
        return SpecState(self.val.copy(), self.wit.copy(), self.tail.copy())


def spec_start(n, spec):
    """The state of n robots before their first sample: rho = +inf for ALWAYS and RECUR, -inf for EVENTUALLY, UNTIL and STAY; guard
    = +inf; witness = -1; every tail entry +inf for STAY and -inf for RECUR (what an always / an eventually over nothing reads)."""
    C = spec.n_clauses
    val = np.full((int(n), C, 2), np.inf, np.float32)
    tail = np.full((int(n), spec.tail_width), np.inf, np.float32)
    for c, cl in enumerate(spec.clauses):
        if cl[0] not in (SPEC_ALWAYS, SPEC_RECUR):
            val[:, c, 0] = -np.inf
        if cl[0] == SPEC_RECUR:
            tail[:, spec.tail_offsets[c]:spec.tail_offsets[c] + spec.holds[c]] = -np.inf
    return SpecState(val, np.full((int(n), C), -1, np.int32), tail)


def spec_check_state(state, n, spec):
    if not isinstance(state, SpecState):
        raise TypeError(f"a specification's state must be a SpecState (spec_start), not {type(state).__name__}")
    if state.val.shape != (n, spec.n_clauses, 2):
        raise ValueError(f"the specification's state is for {state.val.shape[:2]} (robots, clauses), the call has {(n, spec.n_clauses)}")
    if state.tail.shape != (n, spec.tail_width):
        raise ValueError(f"the specification's state has a tail of shape {state.tail.shape}, the nested clauses need {(n, spec.tail_width)}")


def spec_predicate(margins, counts, pred):
    """The value of a predicate (lo, hi, outside) at one sample: margins [n, R], counts [n] regions of each robot's scene.  u = the
    maximum of the margins lo .. min(hi, count) - 1, taken by explicit > in ascending order (-inf for an empty range); the value is
    u for inside, -u for outside."""
    lo, hi, out = pred
    u = np.full(margins.shape[0], -np.inf, np.float32)
    for r in range(lo, min(hi, margins.shape[1])):
        m = margins[:, r]
        take = (r < counts) & (m > u)
        u = np.where(take, m, u)
    return -u if out else u


def spec_mate_predicate(xy, team_size, pred):
    """The value of a mate predicate at one sample: xy [n, 2] float32, n a multiple of team_size.  Per robot i and mate j, m
    ascending: g = d - sqrt(dx * dx + dy * dy), dx = px_i - px_j, every operation float32 and rounded on its own (the circle
    margin of region_margins with the mate as the centre).  together: the minimum by explicit < from +inf; apart: minus the
    maximum by explicit > from -inf."""
    f32 = np.float32
    _, kind, d = pred
    xy = np.asarray(xy, f32)
    n, size = xy.shape[0], int(team_size)
    mates = xy.reshape(n // size, size, 2)
    me = np.arange(n) % size
    u = np.full(n, np.inf if kind == SPEC_PRED_TOGETHER else -np.inf, f32)
    for m in range(size):
        other = np.repeat(mates[:, m], size, axis=0)                    # [n, 2]: mate m of every robot's team
        dx, dy = xy[:, 0] - other[:, 0], xy[:, 1] - other[:, 1]
        g = (f32(d) - np.sqrt(dx * dx + dy * dy)).astype(f32)
        take = (me != m) & ((g < u) if kind == SPEC_PRED_TOGETHER else (g > u))
        u = np.where(take, g, u)
    return u if kind == SPEC_PRED_TOGETHER else -u


def spec_fold(state, path, spec, step0=0):
    """The state after the samples of one call: `path` [T+1][n][P] as follow_waypoints returns it with path_stride=1 (record 0 the
    position at entry, record r the position after r steps of the call).  With step0 == 0 the records 0 .. T are the samples tau =
    0 .. T; with step0 > 0 record 0 is skipped -- the previous call folded it as its last -- and the records 1 .. T are tau = step0
    + 1 .. step0 + T.  Only x and y are used (a missing y is 0).

    Idle robots.  The device kernels (csrc/kernels_follow.h: follow_start / resume start write record 0 for every robot,
    follow_env_step writes record t + 1 after each step, follow_finish fills every record after a robot's last step with the
    position it stands at) and the host loop (`path[ran + 1:, i] = pos`) leave no row unwritten: a robot that is finished, stalled,
    without waypoints or parked in an earlier call holds its position in every record of the call.  The monitor samples whatever
    position the row holds: a parked robot is still somewhere, and its clauses go on being folded.

    The sample at tau with predicate values v1 (and v2), folded per robot and clause, comparisons explicit and strict so that the
    first attainment is kept:
      ALWAYS      if a <= tau <= b and v1 < rho: rho = v1, witness = tau
      EVENTUALLY  if a <= tau <= b and v1 > rho: rho = v1, witness = tau
      UNTIL       at every tau: if v1 < guard: guard = v1;  then if a <= tau <= b: w = v2 if v2 < guard else guard; if w > rho:
                  rho = w, witness = tau  (so pred1 is held from tau = 0 through tau inclusive)
    and for the nested clauses, h the clause's hold, the window the last h + 1 values v1(tau - h) .. v1(tau) (the carried tail and
    this sample's value):
      STAY        if tau >= h and a <= tau - h <= b: s = the window's minimum; if s > rho: rho = s, witness = tau - h
      RECUR       if tau >= h and a <= tau - h <= b: s = the window's maximum; if s < rho: rho = s, witness = tau - h
    The inner extremum is taken under the total order on float32 bits (spec_key: -0.0 < +0.0), the outer comparison is the float
    comparison of the flat clauses; guard is not used and stays +inf.  A window the run ends before completing is never folded;
    the tail then carries its values into the next call.  After every sample the tail is the last h values, oldest first.

    Things that move.  With a MovingRegions the margins of the sample at tau are those of the frame regions.frame_at(tau) =
    f(max(tau - 1, 0)): it depends on the global tau only, so a split run ends on the same bits, and F == 1 is the static Regions
    bit for bit.  A mate predicate's value is spec_mate_predicate of this sample's record, idle mates included; a robot count
    that spec.team_size does not divide is refused.
    Returns a new SpecState."""
    path = np.asarray(path)
    if path.ndim != 3 or path.shape[0] < 2 or not 1 <= path.shape[2] <= 3:
        raise ValueError(f"path must be [T + 1][n][P] with T >= 1 and P in 1 .. 3, got shape {path.shape}")
    if not np.all(np.isfinite(path)):
        raise ValueError("path holds non-finite positions")
    path = path.astype(np.float32)
    T, n, P = path.shape[0] - 1, path.shape[1], path.shape[2]
    step0 = int(step0)
    if step0 < 0 or step0 + T > SPEC_OPEN:
        raise ValueError("step0 must be >= 0 and step0 + T fit an int32")
    reg = spec.regions
    spec.check_robots(n)
    spec_check_state(state, n, spec)
    sc = np.zeros(n, np.int64) if reg.scene is None else reg.scene.astype(np.int64)
    kinds, counts = reg.kinds[sc], reg.counts[sc]
    rows = None if spec.moving else reg.table[sc]
    val, wit, tail = state.val.copy(), state.wit.copy(), state.tail.copy()
    xy = np.zeros((n, 2), np.float32)
    rows_n = np.arange(n)
    for r in range(0 if step0 == 0 else 1, T + 1):
        tau = step0 + r
        xy[:, :min(P, 2)] = path[r, :, :2]
        m = region_margins(xy, reg.table[sc, reg.frame_at(tau)] if spec.moving else rows, kinds)

        def value(pred):
            return spec_mate_predicate(xy, spec.team_size, pred) if _is_mate_predicate(pred) else spec_predicate(m, counts, pred)
        for c, (op, a, b, p1, p2) in enumerate(cl[:5] for cl in spec.clauses):
            rho, guard = val[:, c, 0], val[:, c, 1]
            v1 = value(p1)
            window = a <= tau <= b
            if op in (SPEC_STAY, SPEC_RECUR):
                h, o = spec.holds[c], spec.tail_offsets[c]
                win = np.concatenate([tail[:, o:o + h], v1[:, None].astype(np.float32)], axis=1)   # v1(tau - h) .. v1(tau)
                tail[:, o:o + h] = win[:, 1:]
                if not (tau >= h and a <= tau - h <= b):
                    continue
                key = spec_key(win)
                new = win[rows_n, np.argmin(key, axis=1) if op == SPEC_STAY else np.argmax(key, axis=1)]
                take = (new > rho) if op == SPEC_STAY else (new < rho)
                val[:, c, 0] = np.where(take, new, rho)
                wit[:, c] = np.where(take, tau - h, wit[:, c])
                continue
            if op == SPEC_UNTIL:
                guard = np.where(v1 < guard, v1, guard)
                val[:, c, 1] = guard
                v2 = value(p2)
                w = np.where(v2 < guard, v2, guard)
                take = (w > rho) if window else np.zeros(n, bool)
                new = w
            else:
                take = ((v1 < rho) if op == SPEC_ALWAYS else (v1 > rho)) if window else np.zeros(n, bool)
                new = v1
            val[:, c, 0] = np.where(take, new, rho)
            wit[:, c] = np.where(take, tau, wit[:, c])
    return SpecState(val, wit, tail)


def spec_result(state, spec):
    """The verdict so far, from the carried state: spec_rho [n][C] float32, spec_witness [n][C] int32, robustness [n] float32 (the
    minimum over the clauses by strict <, ascending), weakest [n] int32 (the clause at that minimum), satisfied [n] bool
    (robustness > 0: a margin of exactly 0 is not satisfied).  An EVENTUALLY whose window has not opened reads -inf."""
    rho = state.val[:, :, 0].copy()
    n, C = rho.shape
    if C != spec.n_clauses:
        raise ValueError(f"the state has {C} clauses, the specification {spec.n_clauses}")
    rob, weak = rho[:, 0].copy(), np.zeros(n, np.int32)
    for c in range(1, C):
        take = rho[:, c] < rob
        rob, weak = np.where(take, rho[:, c], rob), np.where(take, c, weak).astype(np.int32)
    return {"spec_rho": rho, "spec_witness": state.wit.copy(), "robustness": rob.astype(np.float32), "weakest": weak,
            "satisfied": rob > 0}


# ---- a plan from a specification: avoid clauses become obstacles, reach clauses stations; per robot the order of
# the stations (Held-Karp over the stations' own cost-to-go fields, with windows and dwell) and the stitched waypoints.  This
# project's own rule, all integers except the two margin tests; the device (csrc/kernels_plan_spec.h: k_plan_region_occupancy,
# k_plan_station, k_plan_tour_matrix, k_plan_tour, k_plan_tour_path, with k_plan_occupancy and k_plan_field as they are; from the
# middle of a run csrc/kernels_plan_spec_resume.h: k_plan_tour_resume, k_plan_tour_path_legs) is held to it bit for bit.  NOT planned:
# smoothing of the legs, mates planning around each other, moving hazards or regions, precedence (until), recurring visits, credit
# for a dwell in progress, more than PLAN_TOUR_STATIONS_MAX stations.
PLAN_TOUR_STATIONS_MAX = 8          # 256 subsets of stations: the tour table of one robot fits a wave's LDS
PLAN_TOUR_TICKS_MAX = 1 << 24       # every open, close and dwell in ticks is clamped here: 8 legs of them stay below 2^30
PLAN_TOUR_INF = 0x3FFFFFFF          # "no feasible way" in the tour table
SPEC_PLAN_KEYS = ("waypoints", "n_waypoints", "count", "status", "cost", "tour_order", "tour_eta", "station_waypoint", "release",
                  "station_cell", "station_margin", "matrix")


def spec_plan_parse(spec):
    """The plannable fragment of a Spec -> (avoid [(lo, hi)], stations [(lo, hi, a, b, hold)]), stations in clause order.
    Avoid: Spec.always(outside(lo, hi)) with the window exactly [0, open].  Station: Spec.eventually(inside(lo, hi), a, b) (hold 0)
    or Spec.stay(inside(lo, hi), hold, a, b).  Everything else is a ValueError naming the clause and the reason: until, recur, an
    always with another window or over inside, an eventually / stay over outside, mate predicates, team_size != 1, MovingRegions,
    no station at all, more than PLAN_TOUR_STATIONS_MAX stations."""
    if not isinstance(spec, Spec):
        raise TypeError(f"spec must be a mobrob_amd.envs.goal_rules.Spec, not {type(spec).__name__}")
    if spec.moving:
        raise ValueError("spec_plan: MovingRegions are not planned for (a plan needs static regions)")
    if spec.team_size != 1:
        raise ValueError(f"spec_plan: team_size must be 1, got {spec.team_size} (teams are not planned from a specification)")
    avoid, stations = [], []
    for c, cl in enumerate(spec.clauses):
        op, a, b, p1 = cl[:4]
        if op == SPEC_UNTIL:
            raise ValueError(f"spec_plan: clause {c}: until is not plannable (precedence between stations is not built)")
        if op == SPEC_RECUR:
            raise ValueError(f"spec_plan: clause {c}: recur is not plannable (a station is visited once)")
        if _is_mate_predicate(p1):
            raise ValueError(f"spec_plan: clause {c}: a mate predicate (together / apart) is not plannable")
        lo, hi, out = p1
        if op == SPEC_ALWAYS:
            if not out:
                raise ValueError(f"spec_plan: clause {c}: always over inside() is not plannable (only always(outside(...)) is: an obstacle)")
            if (a, b) != (0, SPEC_OPEN):
                raise ValueError(f"spec_plan: clause {c}: always(outside(...)) must have the window [0, open], got [{a}, {b}] "
                                 "(an obstacle holds for the whole plan)")
            avoid.append((lo, hi))
        else:
            if out:
                raise ValueError(f"spec_plan: clause {c}: {'stay' if op == SPEC_STAY else 'eventually'} over outside() is not plannable "
                                 "(a station is inside(...))")
            stations.append((lo, hi, a, b, cl[5] if op == SPEC_STAY else 0))
    if not stations:
        raise ValueError("spec_plan: the specification has no visit clause (eventually / stay over inside(...)): nothing to plan")
    if len(stations) > PLAN_TOUR_STATIONS_MAX:
        raise ValueError(f"spec_plan: {len(stations)} stations, at most PLAN_TOUR_STATIONS_MAX = {PLAN_TOUR_STATIONS_MAX}")
    return avoid, stations


def spec_plan_pace(pace, stations):
    """-> the checked pace: an integer >= 1 (at most 2^20); None is 1 where no station has a window or a dwell and a ValueError
    naming `pace` where one has (the plan cannot turn steps into moves without it)"""
    if pace is None:
        if any((a, b, hold) != (0, SPEC_OPEN, 0) for _, _, a, b, hold in stations):
            raise ValueError("spec_plan: pace= is required when a station has a window or a dwell (the steps a robot is given for one "
                             "orthogonal move)")
        return 1
    if isinstance(pace, bool) or not isinstance(pace, (int, np.integer)) or not 1 <= pace <= 1 << 20:
        raise ValueError(f"spec_plan: pace must be an integer in 1 .. 2^20, got {pace!r}")
    return int(pace)


def spec_plan_ticks(stations, pace):
    """The stations' windows and dwells in ticks (PLAN_STEP a pace) -> (open_c, close_c, dwell_c) int32 [M]: ceil(5 a / pace),
    floor(5 b / pace) (an open b: the clamp), ceil(5 hold / pace), each clamped to PLAN_TOUR_TICKS_MAX.  ValueError where a window
    holds no tick at this pace (open_c > close_c)."""
    cap = PLAN_TOUR_TICKS_MAX
    open_c = [min(-((-PLAN_STEP * a) // pace), cap) for _, _, a, _, _ in stations]
    close_c = [cap if b == SPEC_OPEN else min((PLAN_STEP * b) // pace, cap) for _, _, _, b, _ in stations]
    dwell_c = [min(-((-PLAN_STEP * h) // pace), cap) for _, _, _, _, h in stations]
    for j, (o, c) in enumerate(zip(open_c, close_c)):
        if o > c:
            raise ValueError(f"spec_plan: station {j}: the window [{stations[j][2]}, {stations[j][3]}] holds no move boundary at pace {pace} "
                             f"(opens at tick {o}, closes at tick {c})")
    return np.array(open_c, np.int32), np.array(close_c, np.int32), np.array(dwell_c, np.int32)


def spec_plan_scene(regions, walls=None, hazards=None):
    """-> (S, scene [n] int32 or None): the regions' scenes, which the walls' and the hazards' must equal where those exist"""
    plan_scene(walls, hazards)
    for what, sc in (("walls", walls), ("hazards", hazards)):
        if sc is None:
            continue
        if sc.n_scenes != regions.n_scenes:
            raise ValueError(f"spec_plan: the regions have {regions.n_scenes} scenes, the {what} {sc.n_scenes}")
        if (sc.scene is None) != (regions.scene is None) or (sc.scene is not None and not np.array_equal(sc.scene, regions.scene)):
            raise ValueError(f"spec_plan: the regions and the {what} must agree on the scene index per robot")
    return regions.n_scenes, regions.scene


def spec_plan_check(grid, walls, hazards, spec, start, goal, K, pace):
    """spec_plan's refusals, by name -> (avoid, stations, ticks, S, scene, start, goal or None (float32), K, pace)"""
    if not isinstance(grid, GridSpec):
        raise TypeError(f"grid must be a mobrob_amd.envs.goal_rules.GridSpec, not {type(grid).__name__}")
    avoid, stations = spec_plan_parse(spec)
    pace = spec_plan_pace(pace, stations)
    ticks = spec_plan_ticks(stations, pace)
    S, scene = spec_plan_scene(spec.regions, walls, hazards)
    start = np.asarray(start, np.float64)
    if start.ndim != 2 or start.shape[0] < 1 or start.shape[1] not in (2, 3):
        raise ValueError(f"spec_plan: start must be [n_robots, 2 or 3], got shape {start.shape}")
    if goal is not None:
        goal = np.asarray(goal, np.float64)
        if goal.shape != start.shape:
            raise ValueError(f"spec_plan: goal must have start's shape {start.shape}, got {goal.shape}")
    if not np.all(np.isfinite(start)) or (goal is not None and not np.all(np.isfinite(goal))):
        raise ValueError("spec_plan: start and goal must be finite")
    for sc in (walls, hazards, spec.regions):
        if sc is not None:
            sc.check_robots(start.shape[0])
    K = int(K)
    if K < 1:
        raise ValueError("spec_plan: max_waypoints must be >= 1")
    return avoid, stations, ticks, S, scene, start.astype(np.float32), None if goal is None else goal.astype(np.float32), K, pace


def _spec_plan_margins(grid, regions, s):
    """region_margins of scene s at every cell centre -> float32 [G * G][R], cell c = iy * G + ix"""
    G = grid.cells
    c = grid.centre(np.arange(G))
    xy = np.stack([np.broadcast_to(c[None, :], (G, G)).reshape(-1), np.broadcast_to(c[:, None], (G, G)).reshape(-1)], axis=1)
    R = regions.max_regions
    return region_margins(xy, np.broadcast_to(regions.table[s], (G * G, R, 4)), np.broadcast_to(regions.kinds[s], (G * G, R)))


def spec_plan_occupancy(grid, walls, hazards, regions, avoid):
    """The blocked map of a plan from a specification, bool [S][G][G]: grid_occupancy of the walls and hazards, OR-ed per scene with
    the avoid regions -- a cell is blocked when a region r of an avoid range, r < counts[scene], has region_margins(centre)[r] >=
    float32(-inflate).  Equality blocks, as for walls."""
    S = regions.n_scenes
    G = grid.cells
    occ = grid_occupancy(grid, walls, hazards) if (walls is not None or hazards is not None) else np.zeros((S, G, G), bool)
    occ = occ.copy()
    edge = np.float32(-grid.inflate_for(walls))
    for s in range(S):
        if not avoid:
            break
        m = _spec_plan_margins(grid, regions, s)
        for lo, hi in avoid:
            for r in range(lo, min(hi, int(regions.counts[s]))):
                occ[s] |= (m[:, r] >= edge).reshape(G, G)
    return occ


def spec_plan_stations(grid, regions, stations, occ):
    """The anchors -> (station_cell int32 [S][M], station_margin float32 [S][M]).  Per scene and station the candidates are the
    unblocked cells, m(c) = spec_predicate(inside(lo, hi)) at the cell's centre; the best cell is the one of the largest spec_key(m),
    the lowest cell index on a tie, and station_margin is its m (-inf without an unblocked cell); it is the anchor when m > 0, else
    the anchor is -1."""
    S, M, G = regions.n_scenes, len(stations), grid.cells
    cell, margin = np.full((S, M), -1, np.int32), np.full((S, M), -np.inf, np.float32)
    for s in range(S):
        mg = _spec_plan_margins(grid, regions, s)
        free = np.nonzero(~occ[s].reshape(-1))[0]
        if free.size == 0:
            continue
        counts = np.full(G * G, regions.counts[s])
        for j, (lo, hi, _, _, _) in enumerate(stations):
            m = spec_predicate(mg, counts, (lo, hi, False))[free]
            best = int(np.argmax(spec_key(m)))                      # argmax: the first, hence the lowest cell, of equal keys
            margin[s, j] = m[best]
            if m[best] > 0:
                cell[s, j] = free[best]
    return cell, margin


def spec_plan_tour(d0, D, E, open_c, close_c, dwell_c):
    """The order of the stations for n robots at once (Held-Karp).  d0 int64 [n][M]: start to station j; D int64 [n][M][M]: station
    i to station j (the robot's scene's); E int64 [n][M]: station i to the goal (zeros without a goal); PLAN_ASSIGN_NONE reads "no
    path".  dep(j, arr) = max(arr, open_c[j]) + dwell_c[j], feasible iff arr is a real cost and max(arr, open_c[j]) <= close_c[j].
    t[{j}][j] = dep(j, d0[j]); t[mask + j][j] = the minimum over the feasible i in mask of dep(j, t[mask][i] + D[i][j]), taken of the
    pair (value, i), so the lowest i wins a tie; the tour ends at the j minimising (t[full][j] + E[j], j).
    -> (feasible bool [n], cost int64 [n], order int32 [n][M], eta int64 [n][M] (ticks on arrival, before max with open_c), depart
    int64 [n][M]); order, eta, depart are -1 and cost -1 where no feasible tour exists."""
    n, M = d0.shape
    return spec_plan_tour_resume(d0, D, E, np.zeros(n, np.int64), open_c, close_c, dwell_c, np.full(n, (1 << M) - 1, np.int64), 0, False)[:5]


def spec_plan_table(d0, D, open_c, close_c, dwell_c, todo, t0):
    """The tour table, the one statement of its recurrence (spec_plan_tour_resume and spec_plan_best fill it here) -> (t int64
    [n][1 << M][M], pred int8 [n][1 << M][M]).  t[V][j] is the earliest departure from station j after visiting exactly the
    stations of V, j last, from the tick t0 on; it is filled for the masks that are subsets of todo[r] only and PLAN_TOUR_INF
    everywhere else.  t[{j}][j] = dep(j, t0 + d0[j]); t[mask + j][j] = the minimum over the feasible i in mask of dep(j, t[mask][i] +
    D[i][j]), taken of the pair (value, i): the lowest i wins a tie, and pred holds it (-1 at a single station)."""
    n, M = d0.shape
    INF, NONE = PLAN_TOUR_INF, PLAN_ASSIGN_NONE
    full = (1 << M) - 1
    todo = np.asarray(todo, np.int64)
    t0 = int(t0)
    t = np.full((n, 1 << M, M), INF, np.int64)
    pred = np.full((n, 1 << M, M), -1, np.int8)

    def dep(j, arr, ok):
        begin = np.maximum(arr, open_c[j])
        return np.where(ok & (begin <= close_c[j]), begin + dwell_c[j], INF)
    for mask in range(1, full + 1):
        sub = (mask & ~todo) == 0                                # the robots whose todo holds this mask
        if not sub.any():
            continue
        for j in range(M):
            if not mask >> j & 1:
                continue
            rest = mask ^ (1 << j)
            if rest == 0:
                t[:, mask, j] = dep(j, t0 + d0[:, j], sub & (d0[:, j] < NONE))
                continue
            best, via = np.full(n, INF, np.int64), np.full(n, -1, np.int8)
            for i in range(M):                                   # ascending: strict < keeps the lowest i of equal values
                if not rest >> i & 1:
                    continue
                val = dep(j, t[:, rest, i] + D[:, i, j], sub & (t[:, rest, i] < INF) & (D[:, i, j] < NONE))
                take = val < best
                best, via = np.where(take, val, best), np.where(take, i, via).astype(np.int8)
            t[:, mask, j], pred[:, mask, j] = best, via
    return t, pred


def spec_plan_tour_resume(d0, D, E, e0, open_c, close_c, dwell_c, todo, t0, partial):
    """spec_plan_tour from the middle of a run: the one statement of the order rule (spec_plan_tour is this with every station to
    do, t0 = 0 and partial off).  todo int [n]: the bit set of the stations robot r still has to visit; t0: the tick the plan starts
    at; e0 int64 [n]: the start to the goal (0 without a goal, PLAN_ASSIGN_NONE: no path).  The table is filled for the masks that
    are subsets of todo[r] only: t[{j}][j] = dep(j, t0 + d0[j]), the recurrence and dep as in spec_plan_tour.
    partial off: the tour visits all of todo[r] and ends at the j of todo[r] minimising (t[todo][j] + E[j], j); with todo[r] == 0
    there is no station leg and the total is t0 + e0 (feasible iff e0 is a real cost).
    partial on: the visited set V, a subset of todo[r], and its last station j are the lexicographic minimum of (popcount(todo) -
    popcount(V), t[V][j] + E[j], V as an integer, j) over the feasible entries; V = 0 is an entry with the total t0 + e0 and j = -1.
    -> (feasible bool [n], cost int64 [n], order int32 [n][M], eta int64 [n][M], depart int64 [n][M], tour_len int32 [n] = |V|,
    dropped int32 [n] = todo & ~V); order, eta and depart are -1 at the positions >= tour_len; without a feasible entry cost is
    -1, tour_len 0 and dropped is todo."""
    n, M = d0.shape
    INF, NONE = PLAN_TOUR_INF, PLAN_ASSIGN_NONE
    full = (1 << M) - 1
    todo = np.asarray(todo, np.int64)
    t0 = int(t0)
    t, pred = spec_plan_table(d0, D, open_c, close_c, dwell_c, todo, t0)
    # the selection: a strict lexicographic < over ascending (V, j) keeps the lowest (V, j) of equal (left out, total)
    rows = np.arange(n)
    left = np.full(n, M + 1, np.int64)                           # stations of todo left out; M + 1: no entry yet
    cost, visit, last = np.full(n, INF, np.int64), np.zeros(n, np.int64), np.full(n, -1, np.int64)
    have = np.array([bin(int(v)).count("1") for v in todo], np.int64)
    empty = (e0 < NONE) & ((todo == 0) | bool(partial))         # V = 0: the goal leg alone (the first entry: V = 0 is the lowest)
    left, cost = np.where(empty, have, left), np.where(empty, t0 + e0, cost)
    for mask in range(1, full + 1):
        cand = ((mask & ~todo) == 0) if partial else (todo == mask)
        if not cand.any():
            continue
        out = have - bin(mask).count("1")
        for j in range(M):
            if not mask >> j & 1:
                continue
            ok = cand & (t[:, mask, j] < INF) & (E[:, j] < NONE)
            tot = np.where(ok, t[:, mask, j] + E[:, j], INF)
            take = ok & ((out < left) | ((out == left) & (tot < cost)))
            left, cost = np.where(take, out, left), np.where(take, tot, cost)
            visit, last = np.where(take, mask, visit), np.where(take, j, last)
    ok = left <= M
    order, eta, depart = np.full((n, M), -1, np.int32), np.full((n, M), -1, np.int64), np.full((n, M), -1, np.int64)
    tour_len = np.where(ok, np.array([bin(int(v)).count("1") for v in visit], np.int64), 0).astype(np.int32)
    for r in rows[ok]:
        mask, j = int(visit[r]), int(last[r])
        for k in range(int(tour_len[r]) - 1, -1, -1):
            order[r, k] = j
            depart[r, k] = t[r, mask, j]
            i = int(pred[r, mask, j])
            eta[r, k] = t0 + d0[r, j] if i < 0 else t[r, mask ^ (1 << j), i] + D[r, i, j]
            mask, j = mask ^ (1 << j), i
    dropped = (todo & ~np.where(ok, visit, 0)).astype(np.int32)
    return ok, np.where(ok, cost, -1), order, eta, depart, tour_len, dropped


SPEC_REPLAN_KEYS = ("tour_len", "dropped", "done")


def spec_plan_clauses(spec):
    """-> int [M]: the clause index of each station, in the clause order spec_plan_parse numbers the stations in"""
    spec_plan_parse(spec)
    return np.array([c for c, cl in enumerate(spec.clauses) if cl[0] != SPEC_ALWAYS], np.int64)


def spec_plan_done(spec, state):
    """-> bool [n][M]: station j is done for robot r iff state.val[r, clause_j, 0] > 0 -- spec_result's strict rule: a margin of
    exactly 0 (either sign) is not done.  state: a SpecState of this specification (spec_check_state).
    Limit: the carried tail of a stay clause, a dwell in progress, is deliberately not read: a robot interrupted in a dwell dwells
    again in full."""
    clauses = spec_plan_clauses(spec)
    if not isinstance(state, SpecState):
        raise TypeError(f"a specification's state must be a SpecState (spec_start), not {type(state).__name__}")
    spec_check_state(state, state.val.shape[0], spec)
    # rho > 0 read off the float32 bits (0 < bits <= those of +inf): the smallest denormal is done even in a process whose float
    # unit has been put into flush-to-zero mode by a library built for fast math
    b = np.ascontiguousarray(state.val[:, clauses, 0]).view(np.int32)
    return (b > 0) & (b <= np.int32(0x7F800000))


def spec_plan_resume_check(spec, n, pace, state, step0, partial):
    """The refusals of spec_plan's state=, step0= and partial=, by name -> (done bool [n][M], todo int32 [n], t0).  `pace` is the
    checked pace with the caller's None kept (spec_plan_pace's 1 is a pace nobody stated).  t0 = ceil(PLAN_STEP * step0 / pace)
    must not exceed PLAN_TOUR_TICKS_MAX: a time in the table is then at most the larger of t0 and an opening, plus 8 dwells and 9
    legs below PLAN_ASSIGN_NONE each -- under 2^24 + 8 * 2^24 + 9 * 2^21 < 2^28, far below 2^30 as before."""
    M = len(spec_plan_clauses(spec))
    if isinstance(step0, bool) or not isinstance(step0, (int, np.integer)) or step0 < 0:
        raise ValueError(f"spec_plan: step0 must be an integer >= 0, got {step0!r}")
    if not isinstance(partial, (bool, np.bool_)):
        raise ValueError(f"spec_plan: partial must be True or False, got {partial!r}")
    if step0 != 0 and pace is None:
        raise ValueError("spec_plan: pace= is required with a nonzero step0 (the start tick is ceil(PLAN_STEP * step0 / pace))")
    t0 = 0 if step0 == 0 else -((-PLAN_STEP * int(step0)) // int(pace))
    if t0 > PLAN_TOUR_TICKS_MAX:
        raise ValueError(f"spec_plan: step0 = {step0} at pace {pace} starts at tick {t0}, above PLAN_TOUR_TICKS_MAX = {PLAN_TOUR_TICKS_MAX}")
    if state is None:
        done = np.zeros((n, M), bool)
    else:
        spec_check_state(state, n, spec)
        done = spec_plan_done(spec, state)
    todo = ((~done).astype(np.int64) << np.arange(M)).sum(axis=1).astype(np.int32)
    return done, todo, t0


# ---- a team shares the stations: each station to one member, the team done as early as possible.  best is what a
# subset costs a member, spec_plan_share the exact partition of the team's stations among its members; the device
# (csrc/kernels_plan_spec_share.h: k_plan_tour_best, k_plan_team_share, k_plan_team_void) is held to both bit for bit.
SPEC_SHARE_KEYS = ("share", "team_cover", "team_dropped", "team_makespan", "team_total", "team_done")
SPEC_SHARE_OBJECTIVES = ("makespan", "sum")


def spec_plan_share_size(size, objective):
    """The refusals of share= and objective= that need no robot count, by name -> (size, objective)"""
    if isinstance(size, bool) or not isinstance(size, (int, np.integer)) or int(size) not in TEAM_SIZES:
        raise ValueError(f"spec_plan: share must be a team size, one of {TEAM_SIZES}, got {size!r}")
    if objective not in SPEC_SHARE_OBJECTIVES:
        raise ValueError(f"spec_plan: objective must be one of {SPEC_SHARE_OBJECTIVES}, got {objective!r}")
    return int(size), objective


def spec_plan_share_check(n, size, objective):
    """The refusals of spec_plan's share= and objective=, by name -> (size, objective): spec_plan_share_size's, and an n that does
    not split into teams"""
    size, objective = spec_plan_share_size(size, objective)
    if int(n) % size != 0:
        raise ValueError(f"spec_plan: {int(n)} robots do not split into teams of share = {size}")
    return size, objective


def spec_plan_best(d0, D, E, e0, open_c, close_c, dwell_c, T, t0):
    """What every subset of the team's stations costs a robot -> best int64 [n][1 << M].  T int [n]: the bit set of the stations
    the robot's team still has to visit.  With t = spec_plan_table(..., T, t0): best[r][V] = the minimum over the j of V with t[V][j]
    and E[j] real of t[V][j] + E[j] -- the ticks at the end of the robot's best tour over exactly V, goal leg included --,
    best[r][0] = t0 + e0[r] where e0[r] is a real cost, and PLAN_TOUR_INF where nothing is feasible and for every V that is not a
    subset of T[r]."""
    n, M = d0.shape
    INF, NONE = PLAN_TOUR_INF, PLAN_ASSIGN_NONE
    t, _ = spec_plan_table(d0, D, open_c, close_c, dwell_c, T, t0)
    E = np.asarray(E, np.int64)
    tot = np.where((t < INF) & (E[:, None, :] < NONE), t + E[:, None, :], INF)
    best = tot.min(axis=2)
    best[:, 0] = np.where(np.asarray(e0) < NONE, int(t0) + np.asarray(e0, np.int64), INF)
    return best


_SHARE_NONE = 1 << 40   # "no feasible split" in a row of the partition DP: above every sum of sixteen member costs


def _spec_share_pass(best, add, cap):
    """One pass of the partition DP over the members k = 0 .. size - 1 of every team at once.  best int64 [teams][size][256 or
    fewer]; add: the terms are combined by + (else by max); cap int64 [teams] or None: a member's own cost above it is no term.
    row[0][U] = best[0][U]; row[k][U] = the minimum over the V that are subsets of U of combine(row[k - 1][U \\ V], best[k][V]),
    infeasible terms skipped, V ascending and compared by strict <: the lowest V of equal values.
    -> (the last row int64 [teams][W], _SHARE_NONE where nothing is feasible -- a sum of sixteen costs may pass PLAN_TOUR_INF --,
    choice int32 [teams][size][W]: the V taken, 0 where nothing is feasible)"""
    nt, size, W = best.shape
    INF, NO = PLAN_TOUR_INF, _SHARE_NONE
    U = np.arange(W)
    ok = best < INF if cap is None else (best < INF) & (best <= cap[:, None, None])
    row = np.where(ok[:, 0], best[:, 0], NO)
    choice = np.zeros((nt, size, W), np.int32)
    for k in range(1, size):
        new = np.full((nt, W), NO, np.int64)
        for V in range(W):
            sup = U[(U & V) == V]                                    # the U that hold V
            prev, own = row[:, sup ^ V], best[:, k, V][:, None]
            val = prev + own if add else np.maximum(prev, own)
            take = ok[:, k, V][:, None] & (prev < NO) & (val < new[:, sup])
            new[:, sup] = np.where(take, val, new[:, sup])
            choice[:, k, sup] = np.where(take, V, choice[:, k, sup])
        row = new
    return row, choice


def spec_plan_share(best, T, size, objective="makespan", partial=False):
    """The stations of every team allotted to its members, exactly.  best int64 [n][1 << M]: spec_plan_best's; T int [n]: the team's
    stations to visit, the same for every member; size: the team size (TEAM_SIZES; consecutive robots, team r // size, member
    r % size).  -> (share int32 [n]: the bit set of the stations robot r visits, team): team a dict of team_cover, team_dropped
    (int32 bit sets), team_makespan (int32), team_total (int64) and team_feasible (bool), each [n / size].

    Primary pass over the members k and the U that are subsets of T.  "makespan": f[0][U] = best[0][U], f[k][U] = the minimum over
    the subsets V of U of max(f[k - 1][U \\ V], best[k][V]); "sum": the same with +.  Infeasible terms are skipped.
    Covered set C: without partial C = T, and the team is infeasible where f[size - 1][T] is PLAN_TOUR_INF; with partial C is the
    lexicographic minimum of (popcount(T) - popcount(U), f[size - 1][U], U) over the feasible U, and the team is infeasible only
    where no U is feasible.
    Allotment: a sum pass under a cap, which makes (makespan, sum) exact lexicographically.  cap = f[size - 1][C] for "makespan",
    none for "sum" (where f is g and one pass is made).  g[0][U] = best[0][U] where it is <= cap; g[k][U] = the minimum of g[k - 1][U
    \\ V] + best[k][V] over the subsets V of U with best[k][V] <= cap, V ascending and compared by strict <, so that the lowest V
    wins a tie; choice[k][U] is that V.  The backtrack starts at (size - 1, C), and member 0 gets what remains.
    team_makespan is the largest member cost best[r][share[r]], team_total their sum (int64: every cost is below 2^28).  An
    infeasible team: share 0, team_cover 0, team_dropped T, team_makespan and team_total -1."""
    best = np.asarray(best, np.int64)
    n, W = best.shape
    size, objective = spec_plan_share_check(n, size, objective)
    T = np.asarray(T, np.int64)
    if T.shape != (n,) or np.any(T < 0) or np.any(T >= W):
        raise ValueError(f"spec_plan_share: T must be [n] bit sets below {W}")
    nt = n // size
    if np.any(T.reshape(nt, size) != T[::size, None]):
        raise ValueError("spec_plan_share: the members of a team must share one T")
    if not isinstance(partial, (bool, np.bool_)):
        raise ValueError(f"spec_plan: partial must be True or False, got {partial!r}")
    NO = _SHARE_NONE
    Tt, b = T[::size], best.reshape(nt, size, W)
    add = objective == "sum"
    f, choice = _spec_share_pass(b, add, None)
    teams = np.arange(nt)
    if partial:
        pop = np.array([bin(u).count("1") for u in range(W)], np.int64)
        key = (pop[Tt][:, None] - pop[None, :]) << 50 | f << 10 | np.arange(W)[None, :]      # f < 2^32, U < 2^10
        key = np.where(f < NO, key, np.int64(1) << 62)
        C = key.argmin(axis=1)                                                               # the first, hence the lowest, minimum
    else:
        C = Tt.copy()
    feasible = f[teams, C] < NO
    if not add:
        _, choice = _spec_share_pass(b, True, np.where(feasible, f[teams, C], -1))
    share = np.zeros((nt, size), np.int64)
    U = np.where(feasible, C, 0)
    for k in range(size - 1, 0, -1):
        share[:, k] = choice[teams, k, U]
        U = U ^ share[:, k]
    share[:, 0] = U
    cost = np.take_along_axis(b, share[:, :, None], axis=2)[:, :, 0]
    team = {"team_cover": np.where(feasible, C, 0).astype(np.int32), "team_dropped": np.where(feasible, Tt & ~C, Tt).astype(np.int32),
            "team_makespan": np.where(feasible, cost.max(axis=1), -1).astype(np.int32),
            "team_total": np.where(feasible, cost.sum(axis=1), -1).astype(np.int64), "team_feasible": feasible}
    return share.reshape(n).astype(np.int32), team


def spec_team_result(result, spec, size):
    """The team's verdict from the per-robot one (result: a dict with spec_result's spec_rho [n][C]; size: the team size, TEAM_SIZES,
    consecutive robots).  Per clause the team's value is the MAXIMUM over the mates for eventually / stay -- someone did it; strict >
    over ascending members, so the lowest member wins a tie -- and the MINIMUM for always / recur / until -- everyone kept it;
    strict <.  -> team_rho float32 [n / size][C], team_member int32 [n / size][C] (the member, 0 .. size - 1, whose value it is),
    team_robustness float32, team_weakest int32 and team_satisfied bool [n / size] by spec_result's rule (the minimum over the
    clauses by strict <, ascending; satisfied: > 0).  An eventually that no mate's window has opened for reads -inf."""
    if not isinstance(spec, Spec):
        raise TypeError(f"spec must be a mobrob_amd.envs.goal_rules.Spec, not {type(spec).__name__}")
    if isinstance(size, bool) or not isinstance(size, (int, np.integer)) or int(size) not in TEAM_SIZES:
        raise ValueError(f"spec_team_result: size must be one of {TEAM_SIZES}, got {size!r}")
    rho = np.asarray(result["spec_rho"], np.float32)
    if rho.ndim != 2 or rho.shape[1] != spec.n_clauses:
        raise ValueError(f"spec_team_result: spec_rho must be [n][{spec.n_clauses}], got shape {rho.shape}")
    n, C = rho.shape
    size = int(size)
    if n % size != 0:
        raise ValueError(f"spec_team_result: {n} robots do not split into teams of {size}")
    r = rho.reshape(n // size, size, C)
    some = np.array([cl[0] in (SPEC_EVENTUALLY, SPEC_STAY) for cl in spec.clauses])
    val, who = r[:, 0].copy(), np.zeros((n // size, C), np.int32)
    for m in range(1, size):
        take = np.where(some[None, :], r[:, m] > val, r[:, m] < val)
        val, who = np.where(take, r[:, m], val), np.where(take, m, who).astype(np.int32)
    rob, weak = val[:, 0].copy(), np.zeros(n // size, np.int32)
    for c in range(1, C):
        take = val[:, c] < rob
        rob, weak = np.where(take, val[:, c], rob), np.where(take, c, weak).astype(np.int32)
    return {"team_rho": val.astype(np.float32), "team_member": who, "team_robustness": rob.astype(np.float32), "team_weakest": weak,
            "team_satisfied": rob > 0}


def spec_plan(grid, walls, hazards, spec, start, goal=None, K=16, pace=None, *, state=None, step0=0, partial=False, share=None,
              objective="makespan"):
    """The plan of n robots from a specification -> dict.  grid: a GridSpec; walls / hazards: static, or None;
    spec: a Spec of the plannable fragment (spec_plan_parse); start [n][P]; goal [n][P] or None: where every robot ends after its
    last station; K waypoint slots; pace: the steps a robot is given for one orthogonal move (spec_plan_pace).

    Blocked map: spec_plan_occupancy.  Anchors: spec_plan_stations -> station_cell, station_margin [S][M]; covered [S][M] =
    station_margin >= REACH_RADIUS (the tracker calls a waypoint reached within REACH_RADIUS of it: only a covered station is
    certainly entered on arrival).  A scene with an anchor of -1 gives every robot of it status UNREACHABLE.
    Costs: one grid_field per (scene, anchor) and per distinct (scene, goal cell); matrix int32 [S][M][M], matrix[s][i][j] = the field
    of station j at the anchor of station i (-1: none).  Time is in ticks, PLAN_STEP for an orthogonal move and PLAN_DIAG for a
    diagonal one (the fields' units): spec_plan_ticks.  Order: spec_plan_tour.
    Waypoints: the legs in tour order, then the goal leg; each leg descends its target's field by grid_walk_cells' rule (the previous
    direction forgotten at the start of a leg) and emits what grid_path emits: the centres of the cells where the direction
    changes, then the leg's end -- a station's anchor centre, or the goal itself.  z of every waypoint: the goal's, else the start's.
    The dict: waypoints float32 [n][K][P], n_waypoints, count (the waypoints of the full path), status [n] int32 (PLANNED,
    UNREACHABLE: no feasible tour, count 0, TRUNCATED: the first K are written; the device reports UNCONVERGED where a loop hit its
    bound), cost [n] int32 (the ticks at the end, waits included; -1), tour_order int32 [n][M] (the station at each position),
    tour_eta int32 [n][M] (ticks on arrival at each position, before the wait for its opening), station_waypoint int32 [n][M] (the
    index in the full path of each position's anchor waypoint), release int32 [n][K]: at the slot of the waypoint AFTER a station
    whose departure exceeds its arrival, min(ceil(departure ticks * pace / PLAN_STEP), 2^31 - 1), else 0 -- ready for
    Schedule(release), which holds the robot at the station until then --, and station_cell, station_margin, covered, matrix,
    occupancy, open_c, close_c, dwell_c, pace.

    From the middle of a run (state=, step0=, partial=; the outputs SPEC_REPLAN_KEYS).  state: the monitor's SpecState; done
    bool [n][M] = spec_plan_done, and todo[r] is the set of stations not done (all of them without a state): the tour of robot r
    is over todo[r] only, and a missing anchor matters only for a station of todo[r].  step0: the global step the robots stand at;
    the plan starts at tick t0 = ceil(PLAN_STEP * step0 / pace) (at most PLAN_TOUR_TICKS_MAX; pace is then required), and windows,
    cost, tour_eta and release stay absolute: ticks and global steps of the run.  partial: off, every station of todo[r] is visited
    or the robot is UNREACHABLE; on, the largest feasible subset V is (spec_plan_tour_resume) -- a station without an anchor or
    whose window has closed is dropped -- and only no feasible entry at all, not even the goal leg, is UNREACHABLE.  tour_len int32
    [n] = |V|, dropped int32 [n] = the bit set todo & ~V; tour_order, tour_eta and station_waypoint are -1 at the positions >=
    tour_len.  With todo[r] == 0 the plan is the goal leg alone, cost t0 + its ticks; without a goal it is PLANNED with count 0.
    The waypoints and releases are stitched over the tour_len legs and the goal leg by the one loop below.

    A team shares the stations (share=size, objective="makespan" or "sum"; the outputs SPEC_SHARE_KEYS).  Teams
    are Teams' teams: `size` consecutive robots, n a multiple of size.  team_done bool [n / size][M]: a station is done for the team
    once any member's clause reads satisfied; T, the team's stations to visit, is the rest.  spec_plan_best gives what every subset
    of T costs each member, spec_plan_share allots every station of the covered set team_cover to exactly one member -- the
    smallest makespan and under it the smallest sum of the members' costs, or the smallest sum --; with partial the team covers
    the largest set it can and team_dropped is the rest, without it an infeasible team has every member UNREACHABLE with count 0,
    cost -1, orders -1 and share 0.  share int32 [n]: the member's stations; its tour, waypoints and releases are those of todo =
    share[r] with partial off, its cost best[r][share[r]] (a member with an empty share plans the goal leg alone), and its
    dropped is 0 -- the team's loss is team_dropped -- except in a team of one, where it is the team's.  team_makespan int32 and
    team_total int64 [n / size]: the largest member cost and their sum, -1 for an infeasible team.  share=1 is the plan without
    share=, bit for bit, for both objectives; share=None is the call it was.  Mates do not plan around each other.

    Limitations: pace is an estimate of the policy's speed; a robot that arrives later than planned dwells for less time (the
    release is a global step, not a duration); a dwell in progress earns no credit (spec_plan_done); the monitor after the run
    remains the judge."""
    raw_pace = pace
    avoid, stations, (open_c, close_c, dwell_c), S, scene, start, goal, K, pace = spec_plan_check(grid, walls, hazards, spec, start,
                                                                                                 goal, K, pace)
    done, todo, t0 = spec_plan_resume_check(spec, start.shape[0], None if raw_pace is None else pace, state, step0, partial)
    if share is not None:
        share, objective = spec_plan_share_check(start.shape[0], share, objective)
    reg = spec.regions
    n, P = start.shape
    G, M = grid.cells, len(stations)
    occ = spec_plan_occupancy(grid, walls, hazards, reg, avoid)
    cell, margin = spec_plan_stations(grid, reg, stations, occ)
    NONE = PLAN_ASSIGN_NONE
    fields = [[grid_field(occ[s], cell[s, j]).reshape(-1) if cell[s, j] >= 0 else np.full(G * G, -1, np.int32) for j in range(M)]
              for s in range(S)]
    matrix = np.full((S, M, M), -1, np.int32)
    for s in range(S):
        for i in range(M):
            if cell[s, i] >= 0:
                matrix[s, i] = [fields[s][j][cell[s, i]] for j in range(M)]
    sc = np.zeros(n, np.int64) if scene is None else np.asarray(scene, np.int64)
    scell, _ = plan_assign_cells(grid, start, start)
    real = lambda v: np.where(np.asarray(v, np.int64) < 0, NONE, np.asarray(v, np.int64))   # noqa: E731
    d0 = real(np.array([[fields[sc[r]][j][scell[r]] for j in range(M)] for r in range(n)]))
    D = real(matrix)[sc]
    if goal is not None:
        field_of, fcell, fscene = plan_fields(grid, None, scene, goal)
        gfields = [grid_field(occ[fscene[f]], fcell[f]).reshape(-1) for f in range(len(fcell))]
        E = real(np.array([[gfields[field_of[r]][cell[sc[r], i]] if cell[sc[r], i] >= 0 else -1 for i in range(M)] for r in range(n)]))
        e0 = real(np.array([gfields[field_of[r]][scell[r]] for r in range(n)]))
    else:
        E, e0 = np.zeros((n, M), np.int64), np.zeros(n, np.int64)
    # a station without an anchor has a field of -1 everywhere: nothing reaches it or leaves it, so a tour that holds it is infeasible
    ticks = (open_c.astype(np.int64), close_c.astype(np.int64), dwell_c.astype(np.int64))
    shared = {}
    if share is None:
        ok, cost, order, eta, depart, tour_len, dropped = spec_plan_tour_resume(d0, D, E, e0, *ticks, todo, t0, bool(partial))
    else:
        # a station is done for the team once it is for any member; the members' tours are spec_plan_tour_resume's over their shares
        size = share
        team_done = done.reshape(n // size, size, M).any(axis=1)
        T = np.repeat(((~team_done).astype(np.int64) << np.arange(M)).sum(axis=1), size)
        best = spec_plan_best(d0, D, E, e0, *ticks, T, t0)
        mine, team = spec_plan_share(best, T, size, objective, bool(partial))
        ok, cost, order, eta, depart, tour_len, dropped = spec_plan_tour_resume(d0, D, E, e0, *ticks, mine, t0, False)
        lost = ~np.repeat(team["team_feasible"], size)             # an infeasible team: every member UNREACHABLE, nothing planned
        ok, cost, tour_len = ok & ~lost, np.where(lost, -1, cost), np.where(lost, 0, tour_len).astype(np.int32)
        order[lost], eta[lost], depart[lost] = -1, -1, -1
        # a member of a feasible team drops nothing (its share is feasible by construction): the team's loss is team_dropped.  A
        # team of one is the robot, and its loss the robot's -- what spec_plan_tour_resume reports for it without share=
        dropped = np.where(lost, T, np.repeat(team["team_dropped"], size) if size == 1 else 0).astype(np.int32)
        shared = {"share": mine, "team_done": team_done, **team}
    wp, release = np.zeros((n, K, P), np.float32), np.zeros((n, K), np.int32)
    count, status = np.zeros(n, np.int32), np.full(n, UNREACHABLE, np.int32)
    swp = np.full((n, M), -1, np.int32)
    z = (start if goal is None else goal)[:, 2:]

    def centre(c):
        return grid.centre(c % G), grid.centre(c // G)
    for r in np.nonzero(ok)[0]:
        s, cur, cnt = int(sc[r]), int(scell[r]), 0

        def emit(xy, cnt=None):
            if cnt < K:
                wp[r, cnt, :2], wp[r, cnt, 2:] = xy, z[r]
        legs = [(int(cell[s, j]), fields[s][j]) for j in order[r, :tour_len[r]]] + ([] if goal is None else [(None, gfields[field_of[r]])])
        for k, (target, field) in enumerate(legs):
            to = int(fcell[field_of[r]]) if target is None else target
            cells, dirs, st = grid_walk_cells(field.reshape(G, G), occ[s], (cur % G, cur // G), (to % G, to // G))
            if st != PLANNED:
                raise ValueError("spec_plan: a leg of a feasible tour has no walk (the fields are not those of this map)")
            for q in range(1, len(cells) - 1):
                if dirs[q] != dirs[q - 1]:
                    emit(centre(cells[q][1] * G + cells[q][0]), cnt)
                    cnt += 1
            if target is None:
                emit(goal[r, :2], cnt)
            else:
                emit(centre(to), cnt)
                swp[r, k] = cnt
                if depart[r, k] > eta[r, k] and k + 1 < len(legs) and cnt + 1 < K:
                    release[r, cnt + 1] = min(-((-int(depart[r, k]) * pace) // PLAN_STEP), SPEC_OPEN)
            cnt += 1
            cur = to
        count[r], status[r] = cnt, TRUNCATED if cnt > K else PLANNED
    return {"waypoints": wp, "n_waypoints": np.minimum(count, K).astype(np.int32), "count": count, "status": status,
            "cost": cost.astype(np.int32), "tour_order": order, "tour_eta": eta.astype(np.int32), "station_waypoint": swp,
            "release": release, "station_cell": cell, "station_margin": margin, "covered": margin >= np.float32(REACH_RADIUS),
            "matrix": matrix, "occupancy": occ, "open_c": open_c, "close_c": close_c, "dwell_c": dwell_c, "pace": pace,
            "tour_len": tour_len, "dropped": dropped, "done": done, "t0": t0, **shared}
