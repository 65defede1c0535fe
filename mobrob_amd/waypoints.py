"""Waypoint following: a trained goal-conditioned policy as the low-level tracker of a planner's path.

`follow_waypoints(model, env, start, waypoints, ...)` gives every robot a start and a sequence of goals and reports when each
goal is reached.  Two paths, one meaning:
  * device: `env` is a `DeviceGoalVecEnv` -- all robots and steps in ONE engine call (mobrob_ppo_follow_waypoints).
  * host: `env` is an `EnvWrapper` or an env name for `get_env` -- `_host_follow` below, one `model.predict` per robot and
    step.  It is the readable statement of the semantics, and works with any object that has `.predict`.

Per robot (every robot is independent): start at rest on `start`, goal wp[0]; no time limit, no reset.  After each step, if
the robot is inside the reach radius, the step number is its arrival at the waypoint in force and the next waypoint becomes
the goal (pose and velocity kept).  The reach test runs once per step, after the step, so at most one waypoint advances per
step and a robot that starts inside the radius of wp[0] counts after its first step.  After its last waypoint the robot idles;
a robot without waypoints runs no step.

Returned dict (NumPy arrays; n robots, K waypoint slots, P position dimensions):
  arrival [n][K]   1-based arrival step of each waypoint, -1 = not reached
  reached [n]      waypoints reached;  steps [n] steps run;  reward_sum [n] float64 sum of the step rewards (reach bonus included)
  final_distance [n]  distance to the waypoint in force at the end (NaN for a robot without waypoints)
  path [R][n][P]   with path_stride > 0: position after r * path_stride steps (record 0 = start; finished robots stay put)
  trace            the device path's teacher-forcing trace when asked for, else None
  persistent       which device kernel path ran (None on the host)
With `hazards` (a goal_rules.Hazards), also the hazard costs of every step (the reference Engine's constrain_hazards rule at the
position after the step; on the host: info["cost"] of EnvWrapper.step with set_hazards):
  cost_sum [n] float64 sum of the step costs;  violation_steps [n] steps with cost > 0;  first_violation [n] the first such step
  (1-based), -1 = none;  min_clearance [n] smallest (distance - radius) after a step (+inf without hazards, NaN without steps)
`hazards` may be a goal_rules.MovingHazards: F frames of hazards, `frame_steps` steps each.  The check after the step with
0-based global number g -- g = step0 + t, t the step of the call; g = t in a one-shot call -- reads frame f(g) =
min(g // frame_steps, F - 1), or (g // frame_steps) % F with loop=True.  The host loop sets the frame's rows before that step.

With `teams` (a goal_rules.Teams) the robots are partitioned into teams of `size` consecutive robots that must keep `separation`
apart (goal_rules.team_cost states the rule): after every step, each robot that stepped is checked against its team-mates'
positions -- x and y only, as for hazards, for drones too; a mate that did not step (finished, stalled, without waypoints, parked
in an earlier call) counts where it stands; robots of different teams never see each other -- and the dict gains
  team_cost_sum [n] float64 sum of the step costs;  conflict_steps [n] steps with cost > 0;  first_conflict [n] the first such
  step (global, 1-based), -1 = none;  min_team_clearance [n] smallest (distance - separation) to a mate after a step (+inf in a
  team of one, NaN without steps);  closest_partner [n] the mate's robot index at that minimum (-1 = none)
A robot accounts only for the steps in which it stepped itself, so a pair is symmetric only while both move: a parked robot
charges the one that passes it, not itself.  The cost changes nothing else.  A call with teams is always a call of a run.

With `schedule` (a goal_rules.Schedule) the waypoints are TIMED: waypoint k of robot i may not be the goal in force in a step whose
0-based global number g is below release[i][k].  Until then the robot HOLDS at its anchor -- the previous waypoint, `home[i]` (its
start unless given) for k = 0 -- under the policy: it is stepped, observed, path-recorded, hazard- and team-checked as on any step
and counts in `steps`, but a hold step (holding at the step's entry) ignores the reach test, adds nothing to reward_sum and leaves
leg_used as it is.  The goal of step g is a pure function of (k, g), k the waypoints reached: anchor while g < release[i][k], else
waypoint k; it is set before the observation of step g is taken.  The dict gains
  hold_steps [n] hold steps run;  hold_drift [n] the largest distance to the anchor after a hold step (NaN: none);
  lateness [n][K] arrival - release in global steps (NaN: not reached)
and `state.sched` carries the first two.  final_distance is then the distance to the waypoint the robot is on, released or not.
A call with a schedule is always a call of a run; the state holds `release` and `home` (changed by `replan` only), so on a
continued call `schedule=` only says that the run is scheduled.  With every release 0 nothing differs from the run without.

With `walls` (a goal_rules.Walls) every robot that stepped is checked against the axis-aligned boxes of its scene after the step
(goal_rules.wall_check states the rule; x and y only): CONTACT -- the signed distance of the post-step position to each box against
the robot radius -- and CROSSING -- the segment from the pre-step to the post-step position against each closed box, which catches
a step that jumps a thin wall or clips a corner.  Walls are observational: nothing is blocked or deflected.  The dict gains
  wall_cost_sum [n] float64 sum of the step costs;  contact_steps [n] steps with cost > 0;  first_contact [n] the first such step
  (global, 1-based), -1 = none;  min_wall_clearance [n] smallest (signed distance - radius) after a step (+inf without walls, NaN
  without steps);  closest_wall [n] the wall's index at that minimum (-1 = none);  crossing_steps [n] steps whose segment met a
  box;  first_crossing [n] the first such step, -1 = none
and `state.wall` carries the seven.  A call with walls is always a call of a run; `replan` leaves the wall record alone.

With `Walls(..., solid=True)` the walls also BLOCK (goal_rules.wall_block states the rule): inside every step, between the dynamics
and the goal test, the proposed x, y is resolved against the robot's scene -- the robot's centre is kept out of every box inflated
by the radius on each axis; a wall whose inflated box holds the pre-step position does not hold in that step, so a robot that
starts inside one can leave.  The candidates are tried in a fixed order -- the proposed position, the x move alone, the y move
alone, no move -- and the first whose swept segment meets no wall is taken; the velocity of every dropped axis becomes +0.0 (the
robot pushes and slides, it does not bounce).  The reach test, reward, arrival, path and the next observation use the resolved
position; the check above then runs on it and stays observational.  A robot that never had a wall ignored has 0 crossing steps,
and its minimum clearance is > -1e-6 (rounding; exact-0 contacts are not promised).  Not promised: the robot is not placed on the
wall's surface (a gap of up to one step remains), no friction or rotation, robots do not block each other, evaluation takes no
walls.  Solid walls with MovingHazards are refused.  The dict gains
  wall_blocked_steps [n] steps not taken as proposed;  wall_first_blocked [n] the first such step (global, 1-based), -1 = none;
  wall_stopped_steps [n] steps with no move at all;  wall_inside_steps [n] steps in which a wall did not hold
and `state.blocked` carries the four.  Robots stalled against a wall (leg_steps) are replanned by the rounds as any stalled robot.

With `Teams(..., solid=True)` the mates also BLOCK each other (goal_rules.team_block / team_block_step state the rule): a mate is
one more box of the rule above, the closed square of half-width `separation` around where it stands, and with solid walls the
scene's boxes and the mates are resolved at once.  The order is serial inside a team, by team-local index, within one global step:
a member resolves against mates with a lower index where they stand after this step's resolve, against mates with a higher index
where they stood before the step, against a mate that does not step where it stands.  A pair of mates that was never inside each
other's square keeps a Chebyshev distance > separation - 1e-6, so min_team_clearance is > -1e-6 for them.  Not promised: fairness
(the lower index goes first), freedom from deadlock (two mates sent to one point: the first to arrive holds the other out -- the
counters below show it, a leg budget with follow_with_replanning is the remedy, planning with assign= prevents it), anything
across teams.  Runs on the device engine, alone or with solid walls, with or without a schedule; hazards, observational walls
and the host loop are refused by name.  The dict gains
  team_blocked_steps [n] steps blocked by a mate;  team_first_blocked [n] the first such step (global, 1-based), -1 = none;
  team_stopped_steps [n] such steps with no move at all;  team_inside_steps [n] steps inside a mate's square
and `state.team_blocked` carries the four; with solid walls wall_blocked_steps and its kin count the steps a wall blocked.

With `spec` (a goal_rules.Spec) the run is MONITORED: a small specification language over regions (goal_rules.Regions: boxes and
circles; x and y only) is evaluated for every robot from the run's positions -- was the goal region visited inside its window, were
the forbidden regions avoided throughout, was region A kept until B was reached, and by what margin.  A clause is
Spec.always(pred, a, b), Spec.eventually(pred, a, b), Spec.until(pred1, pred2, a, b), Spec.stay(pred, hold, a, b) (inside for hold
consecutive steps) or Spec.recur(pred, every, a, b) (at least once in every window of `every` steps) with predicates inside(lo, hi) / outside(lo,
hi) over a range of regions read as their union and a window [a, b] in sample time tau (global steps completed; tau = 0 is the
start); the specification is the conjunction of its clauses (goal_rules.spec_fold states the fold).  The monitor reads `path`, so
the call needs path_stride=1; it samples whatever position a row holds, and the rows of idle robots hold where they stand.  The
dict gains
  spec_rho [n][C] float32 robustness of each clause so far;  spec_witness [n][C] the sample that decided it (-1: none);
  robustness [n] the smallest clause value;  weakest [n] that clause;  satisfied [n] robustness > 0 (a margin of 0 is not)
and `state.spec` (a goal_rules.SpecState) carries the fold, so a split run ends on the same bits.  On the device the fold is one
kernel over the call's path (PPOEngine.spec_monitor), on the host goal_rules.spec_fold; `monitor(path, spec, ...)` below does either
for a recorded path.  `replan` leaves the monitor alone.  Every other key is what the call without `spec=` returns.  The regions may
move (goal_rules.MovingRegions, from MovingHazards by MovingRegions.from_hazards: the sample at tau reads the frame the run's own
hazard check saw) and a predicate may speak about the team-mates (together(d) / apart(d) with Spec(..., team_size=)): the same
funnel, the same keys.  With `teams=` a spec.team_size above 1 must be teams.size.

Runs.  A planner works in rounds: track for a horizon, look where the robots are, replan the stuck ones, continue.  A RUN is a
sequence of calls over the same robots with the same seed; every call returns `state` (a FollowState: what the robots carry
into the next call) and `status`, and takes the previous call's `state=`.  Call c covers the global steps step0 .. step0 +
max_steps - 1:
  * observation and action noise are drawn per (robot, global step); arrival steps (and first_violation) are global, 1-based;
  * position, velocity, reward sum, steps, waypoints reached (= the index k of the waypoint in force), the arrival row,
    `leg_used` (steps spent on the waypoint in force) and the hazard sums are read at entry and continued, never re-summed: a
    run split into calls ends exactly where one long call ends;
  * leg budget `leg_steps` (0: none, leg_used stays 0): after a step, an arrival sets leg_used = 0, any other step adds 1 to it;
    a robot is active while k < its count and (leg_steps == 0 or leg_used < leg_steps);
  * status [n] at the end of the call: 0 going (the call's step cap ended it), 1 finished, 2 stalled (budget spent), 3 no
    waypoints;
  * between calls `state.replan(rows, waypoints)` gives robots new waypoints: reached = 0, arrival row = -1, leg_used = 0,
    everything else carried;
  * `path` and `trace` are the call's own: record 0 is the position at entry, `steps`, `reached`, `reward_sum` are the run's.
`follow_with_replanning` is that loop with a planner callback.  g is a property of the run, not of the call: with moving
hazards step g sees the same frame in one long call and in any chain of calls, so the split changes nothing here either.  A
planner that holds the `state` a call returned asks `hazards.rows(i, state.step0)` for the scene robot i meets at the next
call's first step (in `follow_with_replanning`, after round r of `horizon` steps, that step is (r + 1) * horizon).
"""
from __future__ import annotations

import numpy as np


def follow_inputs(start, waypoints, n_waypoints=None, pos_dim=None):
    """-> (start [n][P] f32, waypoints [n][K][P] f32, n_waypoints [n] int32), checked.  `waypoints` may be [K][P] (the same
    path for every robot) or [n][K][P] with ragged counts in `n_waypoints`; slots past a robot's count are ignored (zeroed)."""
    start = np.asarray(start, np.float64)
    if start.ndim != 2 or start.shape[0] < 1:
        raise ValueError(f"start must be [n_robots, pos_dim], got shape {start.shape}")
    n, P = start.shape
    if pos_dim is not None and P != int(pos_dim):
        raise ValueError(f"start has {P} position dimensions, the environment {int(pos_dim)}")
    wp = np.asarray(waypoints, np.float64)
    if wp.ndim == 2:
        wp = np.broadcast_to(wp, (n,) + wp.shape)
    if wp.ndim != 3 or wp.shape[0] != n or wp.shape[2] != P or wp.shape[1] < 1:
        raise ValueError(f"waypoints must be [K, {P}] or [{n}, K, {P}] with K >= 1, got shape {np.shape(waypoints)}")
    K = wp.shape[1]
    if n_waypoints is None:
        nw = np.full(n, K, np.int32)
    else:
        nw = np.asarray(n_waypoints)
        if nw.shape != (n,) or not np.issubdtype(nw.dtype, np.integer):
            raise ValueError(f"n_waypoints must be {n} integers, got {nw.dtype} of shape {nw.shape}")
        if np.any(nw < 0) or np.any(nw > K):
            raise ValueError(f"n_waypoints must lie in 0 .. {K}")
        nw = nw.astype(np.int32)
    used = np.arange(K)[None, :] < nw[:, None]
    if not np.all(np.isfinite(start)):
        raise ValueError("start holds non-finite values")
    if not np.all(np.isfinite(wp[used])):
        raise ValueError("waypoints hold non-finite values")
    wp = np.where(used[:, :, None], wp, 0.0)
    return np.ascontiguousarray(start, np.float32), np.ascontiguousarray(wp, np.float32), nw


GOING, FINISHED, STALLED, NO_WAYPOINTS = 0, 1, 2, 3   # status of a robot at the end of a call


class FollowState:
    """What the robots of a run carry from one call into the next (see the module docstring), and the next call's `step0`.
      state [n][6]      position, velocity (unused components zero): float32 from the device, float64 from the host loop
      robot [n][4]      float64 reward sum, steps run, waypoints reached (= index of the waypoint in force), final distance (out only)
      arrival [n][K]    int32 global arrival steps, -1 = not reached;  leg_used [n] int32;  status [n] int32 (of the last call)
      hazard [n][4]     float64 cost sum, violation steps, first violation, min clearance -- or None without hazards
      team [n][5]       float64 team cost sum, conflict steps, first conflict, min clearance to a mate, that mate -- or None
      release [n][K] int32, home [n][P] float32, sched [n][2] float64 hold steps, hold drift -- or None without a schedule
      wall [n][7]       float64 wall cost sum, contact steps, first contact, min clearance, that wall, crossing steps, first
                        crossing -- or None without walls
      blocked [n][4]    int32 blocked steps, first blocked step, fully stopped steps, steps with a wall ignored -- or None unless
                        the walls are solid (`walls` given as the run's Walls, with solid=True)
      team_blocked [n][4] int32 steps blocked by a mate, first such step, fully stopped ones, steps inside a mate's square -- or
                        None unless the teams are solid (`teams` given as the run's Teams, with solid=True)
      spec              a goal_rules.SpecState: the monitor's fold so far -- or None without a specification
      waypoints [n][K][P] float32, n_waypoints [n] int32: the rows in force (changed by `replan` only)"""

    def __init__(self, start, waypoints, n_waypoints=None, hazards=False, pos_dim=None, teams=False, schedule=None, walls=False,
                 spec=None):
        s, wp, nw = follow_inputs(start, waypoints, n_waypoints, pos_dim)
        n, K, P = wp.shape
        self.waypoints, self.n_waypoints, self.step0 = wp, nw, 0
        self.state = np.zeros((n, 6), np.float32)
        self.state[:, :P] = s
        self.robot = np.zeros((n, 4), np.float64)
        self.arrival = np.full((n, K), -1, np.int32)
        self.leg_used, self.status = np.zeros(n, np.int32), np.zeros(n, np.int32)
        self.hazard = np.tile(np.array([0.0, 0.0, -1.0, np.nan]), (n, 1)) if hazards else None
        self.team = np.tile(np.array([0.0, 0.0, -1.0, np.nan, -1.0]), (n, 1)) if teams else None
        self.team_blocked = None
        if getattr(teams, "solid", False):
            from .envs.goal_rules import TEAM_BLOCKED_START
            self.team_blocked = np.tile(np.array(TEAM_BLOCKED_START, np.int32), (n, 1))
        self.wall = None
        if walls:
            from .envs.goal_rules import WALL_START
            self.wall = np.tile(np.array(WALL_START), (n, 1))
        self.blocked = None
        if getattr(walls, "solid", False):
            from .envs.goal_rules import BLOCKED_START
            self.blocked = np.tile(np.array(BLOCKED_START, np.int32), (n, 1))
        self.spec = None
        if spec is not None:
            from .envs.goal_rules import spec_start
            self.spec = spec_start(n, spec)
        self.release = self.home = self.sched = None
        if schedule is not None:
            from .envs.goal_rules import SCHED_START, Schedule
            if not isinstance(schedule, Schedule):
                raise TypeError(f"schedule must be a mobrob_amd.envs.goal_rules.Schedule, not {type(schedule).__name__}")
            self.release, self.home = schedule.for_robots(n, K, s)
            if self.home.shape != (n, P):
                raise ValueError(f"schedule: home must be [{n}, {P}], got shape {self.home.shape}")
            self.release, self.home = self.release.copy(), self.home.copy()
            self.sched = np.tile(np.array(SCHED_START), (n, 1))

    def copy(self):
        c = object.__new__(FollowState)
        from .envs.goal_rules import SpecState
        c.__dict__ = {k: (v.copy() if isinstance(v, (np.ndarray, SpecState)) else v) for k, v in self.__dict__.items()}
        return c

    @property
    def n_robots(self):
        return self.waypoints.shape[0]

    @property
    def positions(self):
        """[n][P] where the robots are"""
        return self.state[:, :self.waypoints.shape[2]]

    @property
    def reached(self):
        return self.robot[:, 2].astype(np.int64)

    def replan(self, rows, waypoints, n_waypoints=None, release=None):
        """New waypoints for the robots `rows` ([m] indices): waypoints [m][K'][P] or [K'][P] (the same for each), counts
        n_waypoints [m] (None: K' each).  Those robots start over on their new rows -- reached = 0, arrival = -1, leg_used = 0 --
        and keep position, velocity, reward sum, steps run, hazard sums, team sums and the wall and blocked records.  K grows when K' is larger.
        In a scheduled run the replanned rows get `release` ([m][K'] or [K'] global steps; None: 0, released at once), their
        `home` becomes where they are, and the hold record is carried.  `release` on a run without a schedule is refused."""
        rows = np.atleast_1d(np.asarray(rows))
        if rows.size == 0:
            return self
        if rows.ndim != 1 or not np.issubdtype(rows.dtype, np.integer) or (rows.size and (rows.min() < 0 or rows.max() >= self.n_robots)):
            raise ValueError(f"replan: rows must be robot indices in 0 .. {self.n_robots - 1}")
        if len(np.unique(rows)) != len(rows):
            raise ValueError("replan: a robot is listed twice")
        n, K, P = self.waypoints.shape
        _, wp, nw = follow_inputs(np.zeros((len(rows), P)), waypoints, n_waypoints, P)
        K2 = wp.shape[1]
        scheduled = getattr(self, "release", None) is not None
        if release is not None:
            if not scheduled:
                raise ValueError("replan: release steps need a run with a schedule (FollowState(..., schedule=Schedule))")
            from .envs.goal_rules import Schedule
            rel = Schedule(release).for_robots(len(rows), K2, np.zeros((len(rows), P)))[0]
        if scheduled and K2 > K:
            self.release = np.concatenate([self.release, np.zeros((n, K2 - K), np.int32)], axis=1)
        if K2 > K:
            self.waypoints = np.concatenate([self.waypoints, np.zeros((n, K2 - K, P), np.float32)], axis=1)
            self.arrival = np.concatenate([self.arrival, np.full((n, K2 - K), -1, np.int32)], axis=1)
        self.waypoints[rows] = 0.0
        self.waypoints[rows, :K2] = wp
        self.n_waypoints[rows] = nw
        self.arrival[rows] = -1
        self.robot[rows, 2] = 0.0
        self.leg_used[rows] = 0
        if scheduled:
            self.release[rows] = 0
            if release is not None:
                self.release[rows, :K2] = rel
            self.home[rows] = self.state[rows, :P]
        return self


def _check_run(state, leg_steps, max_steps, hazards, teams=None, schedule=None, walls=None):
    """The run's values a call is given, checked as the engine checks them (ValueError)."""
    leg_steps = int(leg_steps)
    if leg_steps < 0:
        raise ValueError("leg_steps must be >= 0 (0: no budget)")
    if not isinstance(state, FollowState):
        raise TypeError(f"state must be a FollowState, not {type(state).__name__}")
    if state.step0 < 0 or state.step0 + int(max_steps) > 2 ** 31 - 1:
        raise ValueError("state.step0 must be >= 0 and step0 + max_steps fit an int32")
    if (state.hazard is None) != (hazards is None):
        raise ValueError("a run has hazards in every call or in none (FollowState(..., hazards=True))")
    if (getattr(state, "team", None) is None) != (teams is None):
        raise ValueError("a run has teams in every call or in none (FollowState(..., teams=True))")
    if teams is not None:
        from .envs.goal_rules import Teams
        if not isinstance(teams, Teams):
            raise TypeError(f"teams must be a mobrob_amd.envs.goal_rules.Teams, not {type(teams).__name__}")
        teams.check_robots(state.n_robots)
    team_solid_check(state, hazards, teams, walls)
    if (getattr(state, "wall", None) is None) != (walls is None):
        raise ValueError("a run has walls in every call or in none (FollowState(..., walls=True))")
    if walls is not None:
        from .envs.goal_rules import Walls
        if not isinstance(walls, Walls):
            raise TypeError(f"walls must be a mobrob_amd.envs.goal_rules.Walls, not {type(walls).__name__}")
        walls.check_robots(state.n_robots)
        if np.shape(state.wall) != (state.n_robots, 7):
            raise ValueError("state.wall must be [n_robots][7]")
    solid = walls is not None and bool(getattr(walls, "solid", False))
    if (getattr(state, "blocked", None) is None) == solid:
        raise ValueError("a run has solid walls in every call or in none (FollowState(..., walls=Walls(..., solid=True)))")
    if solid:
        from .envs.goal_rules import MovingHazards
        if isinstance(hazards, MovingHazards):
            raise ValueError("solid=True does not run with MovingHazards yet (static hazards, teams and schedules do)")
        if np.shape(state.blocked) != (state.n_robots, 4):
            raise ValueError("state.blocked must be [n_robots][4]")
    if (getattr(state, "release", None) is None) != (schedule is None):
        raise ValueError("a run has a schedule in every call or in none (FollowState(..., schedule=Schedule))")
    if schedule is not None:
        n, K, P = state.waypoints.shape
        if state.release.shape != (n, K) or state.home.shape != (n, P) or state.sched.shape != (n, 2):
            raise ValueError("state: release, home and sched do not fit the waypoints")
        if np.any(state.release[np.arange(K)[None, :] < state.n_waypoints[:, None]] < 0) or not np.all(np.isfinite(state.home)):
            raise ValueError("state: release steps must be >= 0 and home finite")
        sc = state.sched
        if (np.any(sc[:, 0] < 0) or np.any(sc[:, 0] > state.robot[:, 1]) or np.any(sc[:, 0] != np.floor(sc[:, 0]))
                or np.any(np.isnan(sc[:, 1]) != (sc[:, 0] == 0)) or np.any(sc[:, 1] < 0) or np.any(np.isinf(sc[:, 1]))):
            raise ValueError("state.sched is not a hold record a call returns")
    if not np.all(np.isfinite(state.state)) or not np.all(np.isfinite(state.robot[:, 0])):
        raise ValueError("state holds non-finite positions, velocities or reward sums")
    if np.any(state.leg_used < 0) or np.any(state.leg_used > leg_steps):
        raise ValueError(f"state.leg_used must lie in 0 .. {leg_steps}")
    if np.any(state.robot[:, 2] < 0) or np.any(state.robot[:, 2] > state.n_waypoints):
        raise ValueError("state: waypoints reached must lie in 0 .. n_waypoints")
    return leg_steps


def team_solid_check(state, hazards, teams, walls):
    """The compositions solid teams run in, and the run's team-blocked record: ValueError by name otherwise.  -> solid or not"""
    solid = teams is not None and bool(getattr(teams, "solid", False))
    if (getattr(state, "team_blocked", None) is None) == solid:
        raise ValueError("a run has solid teams in every call or in none (FollowState(..., teams=Teams(..., solid=True)))")
    if solid:
        from .envs.goal_rules import MovingHazards
        if isinstance(hazards, MovingHazards):
            raise ValueError("Teams(solid=True) does not run with MovingHazards yet (solid walls and schedules do)")
        if hazards is not None:
            raise ValueError("Teams(solid=True) does not run with static hazards yet (solid walls and schedules do)")
        if walls is not None and not bool(getattr(walls, "solid", False)):
            raise ValueError("Teams(solid=True) does not run with observational walls yet (Walls(..., solid=True) do)")
        if np.shape(state.team_blocked) != (state.n_robots, 4):
            raise ValueError("state.team_blocked must be [n_robots][4]")
    return solid


def _status(k, nw, leg_used, leg_steps):
    return NO_WAYPOINTS if nw == 0 else FINISHED if k >= nw else STALLED if leg_steps > 0 and leg_used >= leg_steps else GOING


def _solid_step(env, action, pre, rows, radius):
    """EnvWrapper.step with solid walls: the simulator's own step, goal_rules.wall_block on (pre-step xy, proposed xy), the kept
    axes at the simulator's precision and the dropped ones put back with zero velocity, then EnvWrapper.step's tail (reward
    against the goal in force, hazard cost) at the resolved position.  Functionally the rule; not bit-matched to the device.
    -> (reward, info, code, inside)"""
    from .envs import goal_rules as rules
    if not (hasattr(env.env, "pos") and hasattr(env.env, "vel")):
        raise TypeError("solid walls need a simulator whose position and velocity can be set (env.env.pos, env.env.vel)")
    _, _, _, _, info = env.env.step(action)
    prop = np.asarray(env.get_pos(), np.float64)
    _, code, inside = rules.wall_block(pre[:2], prop[:2], rows, radius)
    code = int(code)
    if code:
        vel = np.array(env.env.vel, np.float64)
        for axis, bit in ((0, 2), (1, 1)):               # x is dropped by codes 2 and 3, y by 1 and 3
            if code & bit:
                prop[axis], vel[axis] = pre[axis], 0.0
        env.set_pos(prop)
        env.env.vel = vel
    reward = env.reward_fn()
    hz = getattr(env, "_hazards", None)
    if hz is not None:
        cost, _ = rules.hazard_cost(env.get_pos(), hz.rows(), hz.cost, hz.indicator)
        info = dict(info)
        info["cost_hazards"] = info["cost"] = float(cost)
    return reward, info, code, bool(inside)


def _host_follow(model, make_env, state, max_steps, deterministic, seed, path_stride, hazards=None, leg_steps=0, teams=None,
                 schedule=None, walls=None):
    """The semantics, one robot after another on EnvWrapper's public API (make_env(i) -> the robot's env): one call of the run
    `state` is in (a fresh FollowState: the robots at rest on their starts).  Returns the dict and the state after the call.
    The simulator's noise is seeded per (robot, global step), so a run split into calls draws what one long call draws.
    With `teams` the loop stays robot after robot and keeps every robot's position after each step of the call (where it stands,
    for a step it did not take) and who stepped; after the last robot goal_rules.team_fold applies the rule.  The cost never feeds
    back into a robot's motion, so this equals stepping the robots in lockstep exactly.
    With `schedule` (the state holds release and home) the goal of every step is set per the rule before the step's observation
    is taken, a hold step skips the reward sum, the arrival and the leg count, and goal_rules.schedule_fold folds the hold
    record from the anchors and the float32 positions after the hold steps.
    With `walls` every step's float32 x, y before and after it are kept and goal_rules.wall_fold applies wall_check per step after
    the last robot.  With walls.solid every step is _solid_step (wall_block inside the step) and the blocked record is folded
    by goal_rules.wall_blocked_fold."""
    from .envs.goal_rules import MovingHazards, hazard_cost, schedule_fold, team_fold, wall_blocked_fold, wall_fold
    solid = walls is not None and bool(getattr(walls, "solid", False))
    if teams is not None and bool(getattr(teams, "solid", False)):
        raise ValueError("Teams(solid=True) runs on the device engine only: the host loop steps robot after robot, not step after step")
    st = state.copy()
    st.state = st.state.astype(np.float64)              # the host simulator's own precision, carried exactly
    wp, nw, step0 = st.waypoints, st.n_waypoints, st.step0
    n, K, P = wp.shape
    if hazards is not None:
        hazards.check_robots(n)
    moving = isinstance(hazards, MovingHazards)
    final_distance = np.full(n, np.nan)
    path = np.zeros((max_steps // path_stride + 1, n, P), np.float32) if path_stride > 0 else None
    key = None if seed is None else int(seed) & (2 ** 64 - 1)
    if teams is not None:
        team_xy, team_stepped = np.zeros((max_steps, n, 2)), np.zeros((max_steps, n), bool)
        team_xy[:, :, :min(P, 2)] = st.state[None, :, :min(P, 2)]
    if walls is not None:
        wall_pre, wall_post = np.zeros((max_steps, n, 2), np.float32), np.zeros((max_steps, n, 2), np.float32)
        wall_stepped = np.zeros((max_steps, n), bool)
        wall_code, wall_inside = np.zeros((max_steps, n), np.int64), np.zeros((max_steps, n), bool)
    if schedule is not None:
        rel, home = st.release, st.home
        held, held_anchor, held_pos = np.zeros((max_steps, n), bool), np.zeros((max_steps, n, P), np.float32), np.zeros((max_steps, n, P), np.float32)

    def goal_of(i, k, g):                                # -> (the goal in force of robot i, on waypoint k, in global step g; holding?)
        if schedule is not None and k < nw[i] and g < rel[i, k]:
            return (wp[i, k - 1] if k > 0 else home[i]), True
        return wp[i, k], False
    for i in range(n):
        pos, vel = st.state[i, :P].copy(), st.state[i, 3:3 + P].copy()
        k, leg_used, ran = int(st.robot[i, 2]), int(st.leg_used[i]), 0
        if path is not None:
            path[0, i] = pos
        if k < nw[i] and (leg_steps == 0 or leg_used < leg_steps):
            env = make_env(i)
            if hazards is not None and not moving:
                rows = hazards.rows(i)
                env.set_hazards(rows[:, :2], rows[:, 2], hazards.cost, hazards.indicator)
            if seed is not None:
                env.seed(int(seed) + i)
            env.env.reset()                            # the simulator at rest ...
            env.reset(init_pos=pos)
            if np.any(vel != 0.0):                     # ... then moving as the robot was when the last call ended
                if not hasattr(env.env, "vel"):
                    raise TypeError("resuming a moving robot needs a simulator whose velocity can be set (env.env.vel)")
                env.env.vel = vel.copy()
            goal, hold = goal_of(i, k, step0)
            env.set_goal(goal)
            for t in range(max_steps):
                g = step0 + t                          # the global step
                if moving:                             # the frame in force at the check after this step
                    rows = hazards.rows(i, g)
                    env.set_hazards(rows[:, :2], rows[:, 2], hazards.cost, hazards.indicator)
                if key is not None:
                    env.env.seed([key, i, g])
                obs = env.get_obs()
                a, _ = model.predict(obs, deterministic=deterministic)
                if walls is not None:
                    wall_pre[t, i, :min(P, 2)] = pos[:2]
                if solid:
                    r, info, wall_code[t, i], wall_inside[t, i] = _solid_step(env, a, pos, walls.rows(i), walls.radius)
                else:
                    _, r, _, _, info = env.step(a)
                if not hold:                           # a hold step's reward is progress towards a place the robot waits at
                    st.robot[i, 0] += float(r)
                st.robot[i, 1] += 1
                ran = t + 1
                pos = np.asarray(env.get_pos(), np.float64)[:P]
                if teams is not None:
                    team_xy[t:, i, :min(P, 2)], team_stepped[t, i] = pos[:2], True
                if walls is not None:
                    wall_post[t, i, :min(P, 2)], wall_stepped[t, i] = pos[:2], True
                if hazards is not None:
                    h = st.hazard[i]
                    h[0] += info["cost"]
                    if info["cost"] > 0:
                        h[1] += 1
                        h[2] = g + 1 if h[2] < 0 else h[2]
                    h[3] = min(np.inf if np.isnan(h[3]) else h[3], hazard_cost(pos, rows)[1])
                if path is not None and (t + 1) % path_stride == 0:
                    path[(t + 1) // path_stride, i] = pos
                if hold:                               # no arrival, and waiting is not charged to the leg
                    held[t, i], held_anchor[t, i], held_pos[t, i] = True, goal, pos
                elif env.reached():
                    st.arrival[i, k] = g + 1
                    k, leg_used = k + 1, 0
                    if k == nw[i]:
                        break
                elif leg_steps > 0:
                    leg_used += 1
                    if leg_used >= leg_steps:
                        break
                nxt, hold = goal_of(i, k, g + 1)       # the goal of the next step, set before its observation is taken
                if nxt is not goal and not np.array_equal(nxt, goal):
                    env.set_goal(nxt)
                goal = nxt
            vel = np.asarray(getattr(env.env, "vel", np.zeros(P)), np.float64)[:P]
            if hazards is not None:
                env.set_hazards(None)
        if nw[i] > 0:
            final_distance[i] = float(np.linalg.norm(wp[i, min(k, nw[i] - 1)].astype(np.float64) - pos))
        st.state[i, :P], st.state[i, 3:3 + P] = pos, vel
        st.robot[i, 2], st.robot[i, 3], st.leg_used[i] = k, final_distance[i], leg_used
        st.status[i] = _status(k, nw[i], leg_used, leg_steps)
        if path is not None:
            path[ran // path_stride + 1:, i] = pos
    if teams is not None:
        st.team = team_fold(st.team, team_xy, team_stepped, teams, step0)
    if schedule is not None:
        st.sched = schedule_fold(st.sched, held_anchor, held_pos, held)
    if walls is not None:
        st.wall = wall_fold(st.wall, wall_pre, wall_post, wall_stepped, walls, step0)
    if solid:
        st.blocked = wall_blocked_fold(st.blocked, wall_code, wall_inside, wall_stepped, step0).astype(np.int32)
    st.step0 = step0 + max_steps
    out = {"arrival": st.arrival.astype(np.int64), "reached": st.reached, "steps": st.robot[:, 1].astype(np.int64),
           "reward_sum": st.robot[:, 0].copy(), "final_distance": final_distance, "trace": None, "persistent": None,
           "state": st, "status": st.status.copy()}
    if hazards is not None:
        out.update({"cost_sum": st.hazard[:, 0].copy(), "violation_steps": st.hazard[:, 1].astype(np.int64),
                    "first_violation": st.hazard[:, 2].astype(np.int64), "min_clearance": st.hazard[:, 3].copy()})
    if teams is not None:
        out.update(team_result(st.team))
    if schedule is not None:
        out.update(schedule_result(st))
    if walls is not None:
        out.update(wall_result(st))
    if solid:
        out.update(blocked_result(st))
    if path is not None:
        out["path"] = path
    return out


def wall_result(state):
    """The keys a run with walls adds to a call's dict, from the state after the call (state.wall [n][7])."""
    w = state.wall
    return {"wall_cost_sum": w[:, 0].copy(), "contact_steps": w[:, 1].astype(np.int64), "first_contact": w[:, 2].astype(np.int64),
            "min_wall_clearance": w[:, 3].copy(), "closest_wall": w[:, 4].astype(np.int64), "crossing_steps": w[:, 5].astype(np.int64),
            "first_crossing": w[:, 6].astype(np.int64)}


def blocked_result(state):
    """The keys a run with solid walls adds to a call's dict, from the state after the call (state.blocked [n][4])."""
    b = np.asarray(state.blocked)
    return {"wall_blocked_steps": b[:, 0].astype(np.int64), "wall_first_blocked": b[:, 1].astype(np.int64),
            "wall_stopped_steps": b[:, 2].astype(np.int64), "wall_inside_steps": b[:, 3].astype(np.int64)}


def schedule_result(state):
    """The keys a scheduled run adds to a call's dict, from the state after the call."""
    from .envs.goal_rules import Schedule
    return {"hold_steps": state.sched[:, 0].astype(np.int64), "hold_drift": state.sched[:, 1].copy(),
            "lateness": Schedule.lateness(state.release, state.arrival)}


def team_blocked_result(state):
    """The keys a run with solid teams adds to a call's dict, from the state after the call (state.team_blocked [n][4])."""
    b = np.asarray(state.team_blocked)
    return {"team_blocked_steps": b[:, 0].astype(np.int64), "team_first_blocked": b[:, 1].astype(np.int64),
            "team_stopped_steps": b[:, 2].astype(np.int64), "team_inside_steps": b[:, 3].astype(np.int64)}


def team_result(team):
    """The keys a team record [n][5] adds to a call's dict."""
    return {"team_cost_sum": team[:, 0].copy(), "conflict_steps": team[:, 1].astype(np.int64), "first_conflict": team[:, 2].astype(np.int64),
            "min_team_clearance": team[:, 3].copy(), "closest_partner": team[:, 4].astype(np.int64)}


def monitor(path, spec, step0=0, state=None, engine=None):
    """A specification folded over a recorded path: path [T + 1][n][P] at stride 1 (record 0 the position at entry), step0 the
    global step at the path's entry, state the goal_rules.SpecState of the run so far (None: before the first sample).  With
    `engine` (a PPOEngine, or anything with `.engine`) the fold runs on the device (PPOEngine.spec_monitor), without it is the
    NumPy rule (goal_rules.spec_fold); both give the same bits.  Returns (the new SpecState, the five keys of spec_result)."""
    from .envs.goal_rules import Spec, spec_fold, spec_result, spec_start
    if not isinstance(spec, Spec):
        raise TypeError(f"spec must be a mobrob_amd.envs.goal_rules.Spec, not {type(spec).__name__}")
    if engine is not None:
        return getattr(engine, "engine", engine).spec_monitor(spec, path, step0=step0, state=state)
    if state is None:
        state = spec_start(np.shape(path)[1], spec)
    new = spec_fold(state, path, spec, step0)
    return new, spec_result(new, spec)


def spec_team_result(result, spec, size):
    """The team's verdict of a run with a specification, from a call's dict or monitor()'s (its spec_rho [n][C]): per clause the
    maximum over the `size` mates for eventually / stay -- someone did it -- and the minimum for always / recur / until -- everyone
    kept it.  goal_rules.spec_team_result: team_rho, team_member, team_robustness, team_weakest, team_satisfied, each per team."""
    from .envs.goal_rules import spec_team_result as rule
    return rule(result, spec, size)


def _spec_check_call(spec, path_stride, state):
    """`spec=` of a call: the type, the stride the monitor needs and the run's state.  -> the SpecState at entry, or None (the
    call starts the run: spec_start once the robots are counted)"""
    from .envs.goal_rules import Spec
    if not isinstance(spec, Spec):
        raise TypeError(f"spec must be a mobrob_amd.envs.goal_rules.Spec, not {type(spec).__name__}")
    if int(path_stride) != 1:
        raise ValueError(f"spec= monitors the run from its path: it needs path_stride=1, got path_stride={int(path_stride)}")
    if state is None:
        return None
    carried = getattr(state, "spec", None)
    if carried is None and getattr(state, "step0", 0) != 0:
        raise ValueError("a run is monitored in every call or in none (FollowState(..., spec=Spec), or spec= from the first call on)")
    return carried


def _spec_fold_call(out, spec, carried, step0, engine):
    """Folds the call's own path into the monitor and adds the state and the five keys to the call's dict."""
    new, res = monitor(out["path"], spec, step0=step0, state=carried, engine=engine)
    out["state"].spec = new
    out.update(res)
    return out


def follow_waypoints(model, env, start=None, waypoints=None, n_waypoints=None, *, max_steps=1000, deterministic=True, seed=0,
                     path_stride=0, hazards=None, state=None, leg_steps=0, teams=None, schedule=None, walls=None, spec=None):
    """Every robot i follows waypoints[i][:n_waypoints[i]] from start[i] under `model` (a PPO, or for the host path anything
    with `.predict`).  `env`: a DeviceGoalVecEnv (device path), an EnvWrapper, or an env name for `get_env` (host path; a
    fresh environment per robot for a name, the given one reused robot after robot otherwise).  Returns the dict described in
    the module docstring.  hazards: a goal_rules.Hazards or MovingHazards (hazard costs, see the module docstring).
    state: the `state` a previous call returned -- this call continues that run (start / waypoints / n_waypoints must then be
    None: the robots are where they were, on the waypoints the state holds).  leg_steps: step budget per waypoint (0: none).
    teams: a goal_rules.Teams (separation costs between team-mates, see the module docstring).
    schedule: a goal_rules.Schedule (release steps and holds, see the module docstring); with `state`, which holds the release
    steps in force, it only says that the run is scheduled.
    walls: a goal_rules.Walls (box contact and crossing checks, see the module docstring).
    spec: a goal_rules.Spec (the run is monitored, see the module docstring); needs path_stride=1."""
    from .envs.vec_env import DeviceGoalVecEnv
    from .envs.wrapper import EnvWrapper, TimeLimit, get_env
    max_steps, path_stride = int(max_steps), int(path_stride)
    if max_steps < 1 or path_stride < 0:
        raise ValueError("max_steps must be >= 1 and path_stride >= 0")
    if state is not None and not (start is None and waypoints is None and n_waypoints is None):
        raise ValueError("a resumed call takes its robots and waypoints from `state` (new waypoints: state.replan)")
    if state is None and (start is None or waypoints is None):
        raise ValueError("start and waypoints are needed unless `state` continues a run")
    if spec is None and getattr(state, "spec", None) is not None:
        raise ValueError("a run is monitored in every call or in none: state.spec is set, spec= is missing")
    carried = None if spec is None else _spec_check_call(spec, path_stride, state)
    if spec is not None and teams is not None and spec.team_size > 1 and teams.size != spec.team_size:
        raise ValueError(f"teams.size = {teams.size} differs from spec.team_size = {spec.team_size}: a mate predicate speaks about the run's teams")
    if isinstance(env, DeviceGoalVecEnv):
        if state is None:
            state = FollowState(start, waypoints, n_waypoints, hazards is not None, env.pos_dim, teams if teams is not None else False, schedule,
                                walls if walls is not None else False)
        _check_run(state, leg_steps, max_steps, hazards, teams, schedule, walls)
        if spec is not None:
            spec.check_robots(state.n_robots)
        out = env.follow(getattr(model, "engine", model), max_steps=max_steps, deterministic=deterministic, seed=seed,
                         path_stride=path_stride, hazards=hazards, resume=state, leg_steps=leg_steps, teams=teams,
                         schedule=schedule, walls=walls)
        return out if spec is None else _spec_fold_call(out, spec, carried, state.step0, getattr(model, "engine", model))
    if isinstance(env, str):
        name = env

        def make_env(i):
            return get_env(name, terminate_on_goal=False)
        pos_dim = make_env(0).env.pos_dim
    else:
        while isinstance(env, TimeLimit):                # no time limit
            env = env.env
        if not isinstance(env, EnvWrapper):
            raise TypeError(f"follow_waypoints: env must be a DeviceGoalVecEnv, an EnvWrapper or an env name, not {type(env).__name__}")
        pos_dim = len(env.get_pos())

        def make_env(i):
            return env
    if state is None:
        state = FollowState(start, waypoints, n_waypoints, hazards is not None, pos_dim, teams if teams is not None else False, schedule,
                            walls if walls is not None else False)
    elif isinstance(state, FollowState) and state.waypoints.shape[2] != pos_dim:
        raise ValueError(f"state has {state.waypoints.shape[2]} position dimensions, the environment {pos_dim}")
    leg_steps = _check_run(state, leg_steps, max_steps, hazards, teams, schedule, walls)
    if spec is not None:
        spec.check_robots(state.n_robots)
    out = _host_follow(model, make_env, state, max_steps, deterministic, seed, path_stride, hazards, leg_steps, teams, schedule,
                       walls)
    return out if spec is None else _spec_fold_call(out, spec, carried, state.step0, None)   # two paths, one meaning: spec_fold


def follow_with_replanning(model, env, start, waypoints, planner, *, horizon, rounds, leg_steps=0, n_waypoints=None,
                           deterministic=True, seed=0, hazards=None, teams=None, schedule=None, walls=None, spec=None, path_stride=0):
    """A planner's loop around the tracker: `rounds` calls of `horizon` steps each, one run (see the module docstring).  After
    every round but the last, `planner(positions [n][P], status [n], reached [n])` returns {robot index: new waypoints [k][P]}
    (or None / {} for no change), applied through FollowState.replan.  The loop ends early once no robot is going or stalled
    and the planner changes nothing.  Returns the last call's dict plus `round_status` [rounds run][n].  teams: a
    goal_rules.Teams; the planner callback is unchanged (the team sums are in the returned dict and in its `state`).  schedule: a
    goal_rules.Schedule; a planner that returns {robot: (waypoints, release)} gives the new waypoints release steps (global).
    walls: a goal_rules.Walls; replanning leaves the wall record alone.  spec: a goal_rules.Spec -- the run is monitored round
    after round (needs path_stride=1; `path` is then the last round's) and replanning leaves the monitor alone: a planner whose
    attribute `wants_state` is true (GridPlanner.spec_callback) is called as planner(positions, status, reached, state=the run's
    FollowState) and may READ the monitor's carried state (state.spec, state.step0) to leave out what is already achieved; nothing
    writes it.  Every other planner is called as before.  When such a planner returns releases the run needs a schedule from its
    first call (schedule=): a ValueError naming it where there is none."""
    horizon, rounds = int(horizon), int(rounds)
    if spec is not None:
        _spec_check_call(spec, path_stride, None)
    if horizon < 1 or rounds < 1:
        raise ValueError("horizon and rounds must be >= 1")
    out, state, statuses = None, None, []
    for r in range(rounds):
        first = state is None
        out = follow_waypoints(model, env, start if first else None, waypoints if first else None, n_waypoints if first else None,
                               max_steps=horizon, deterministic=deterministic, seed=seed, hazards=hazards, state=state,
                               leg_steps=leg_steps, teams=teams, schedule=schedule, walls=walls, spec=spec, path_stride=path_stride)
        state = out["state"]
        statuses.append(out["status"].copy())
        if r + 1 == rounds:
            break
        if getattr(planner, "wants_state", False):
            plan = planner(np.array(state.positions), out["status"].copy(), out["reached"].copy(), state=state) or {}
            if schedule is None and any(isinstance(w, tuple) and np.any(np.asarray(w[1]) != 0) for w in plan.values()):
                raise ValueError("follow_with_replanning: the planner returned release steps but the run has no schedule; pass "
                                 "schedule= (a goal_rules.Schedule, e.g. the first plan's or Schedule(zeros)) from the first call")
        else:
            plan = planner(np.array(state.positions), out["status"].copy(), out["reached"].copy()) or {}
        for robot, w in plan.items():
            if schedule is None and isinstance(w, tuple) and getattr(planner, "wants_state", False):
                w = w[0]                                             # releases all zero: released at once, as without a schedule
            if schedule is not None and isinstance(w, tuple):
                state.replan([int(robot)], np.asarray(w[0], np.float64)[None], release=np.asarray(w[1])[None])
            else:
                state.replan([int(robot)], np.asarray(w, np.float64)[None])
        if not plan and not np.any((out["status"] == GOING) | (out["status"] == STALLED)):
            break
    out["round_status"] = np.stack(statuses)
    return out
