"""Grid planner: from an arena described with `goal_rules.Walls` / `goal_rules.Hazards` and a goal per robot to the waypoints the
tracker (`mobrob_amd.waypoints`) follows.

    planner = GridPlanner(env, walls=W, hazards=H, cells=64)
    plan = planner.plan(start, goal)                          # all robots in one device call
    follow_with_replanning(model, env, start, plan["waypoints"], planner.callback(goal), n_waypoints=plan["n_waypoints"], ...)

The rule -- grid, blocked cells, cost-to-go field, path, waypoints -- is stated once in NumPy (goal_rules.GridSpec, grid_occupancy,
grid_field, grid_path).  Two paths, one meaning, bit for bit:
  * device: `env` is a `DeviceGoalVecEnv` and `engine` a PPOEngine (or a PPO that has one): mobrob_ppo_plan_grid, three kernels.
  * host: `env` is an `EnvWrapper` or an env name: the NumPy rule itself (as `_host_follow` serves following).
Line-of-sight smoothing (`smooth=True`): of the walk's cells only those a straight leg cannot skip become waypoints
(goal_rules.grid_los, grid_smooth; device: mobrob_ppo_plan_smooth on the resident fields, k_plan_smooth in k_plan_path's place).
Moving hazards (`hazards=MovingHazards(...)`, `layer_steps=`): the plan is made over time -- layers of occupancy, one
per action of `layer_steps` steps, a wait where waiting for a hazard to pass is cheapest -- and carries `release` steps and a
`schedule` for the tracker (goal_rules.grid_plan_time; device: mobrob_ppo_plan_grid_time).  Teams (`teams=Teams(...)`, DESIGN
4.12.3): inside a team the members plan in index order and every member's walk is reserved in the layers of the members after it,
so mates are planned around each other (goal_rules.grid_plan_team; device: mobrob_ppo_plan_grid_team).  Smoothing over time
(`time_smooth=True`): a straight leg is kept only where it is clear in EVERY layer it spans, so a leg of two or more
actions is clear whatever the robot's speed along it, and the plan holds the robot at every anchor until the leg's first layer
(goal_rules.grid_plan_time(smooth=True); device: mobrob_ppo_plan_grid_time_smooth).  With teams a kept leg is at
most `max_leg` actions long and is reserved for the later members as a swept region, all of its cells in every layer of its span
(goal_rules.grid_plan_team(smooth=True); device: mobrob_ppo_plan_grid_team_smooth).  Reordering rounds (`retries=R`, DESIGN
4.12.6): a team whose plan leaves members parked is planned again, inside the same call, with those members first, and the plan
with the fewest parked members is the result (goal_rules.grid_plan_team_rounds; device: mobrob_ppo_plan_grid_team_rounds).  Goal
assignment (`assign="sum"` or `"makespan"`): a team is given places to occupy, not a pairing -- in front of the
team plan, every team's members and goals are matched at minimum cost on each robot's own static cost-to-go, and the plan is made
for the assigned goals, through whichever team path the planner is configured for; `planner.assign(start, goal)` is that step on
its own (goal_rules.grid_assign; device: mobrob_ppo_plan_assign).  Clearance (`clearance=(reach, weight)`): a static
plan that pays a surcharge for entering a cell within `reach` cells of a blocked one, so it takes the middle of a corridor where
that costs little (goal_rules.grid_plan(..., clearance=); device: mobrob_ppo_plan_grid_clear, mobrob_ppo_plan_smooth_clear).
A plan from a specification (`planner.plan_spec(start, spec, goal=None, pace=None)`): the avoid clauses of a
goal_rules.Spec become obstacles, its reach clauses stations, and per robot the visit order and the stitched waypoints are chosen
(goal_rules.spec_plan; device: mobrob_ppo_spec_plan).
Walls as solid bodies are not planned for."""
from __future__ import annotations

import numpy as np

from .envs import goal_rules as rules


_UNSET = object()   # max_leg= not given


class GridPlanner:
    """A planner over one scene.  env: a DeviceGoalVecEnv (device path; `engine`: the PPOEngine or PPO to run on), or an env name
    / EnvWrapper (host path, the NumPy rule).  walls / hazards: goal_rules.Walls / Hazards or None; cells: 32, 64 or 128 per side
    over the env's [-extent, extent]^2; inflate: clearance of a blocked cell's centre (None: the walls' radius + one cell);
    max_waypoints: the K slots of a plan.  smooth: line-of-sight smoothing of every plan (plan(..., smooth=) overrides it per
    call); los_margin: 0 or 1, the cells a smoothed leg keeps clear on either side (1: a leg of two or more moves is as far from
    walls as the unsmoothed path, also on the first leg from an off-centre start; but a walk ALONG blocked cells has no clear
    cell to see from and keeps every cell as a waypoint -- in cluttered scenes or with a small inflate use 0).
    hazards may be a goal_rules.MovingHazards: every plan is then a time plan.  layer_steps (required then): the steps a robot is
    given for one move or wait; layers: the actions planned in time before the conservative tail.  Nothing of a time plan stays
    resident, so every call computes.  time_smooth: line-of-sight smoothing of every time plan, with los_margin, each leg tested
    against every layer it spans (plan(..., time_smooth=) overrides it per call); it belongs to moving hazards or teams of two or
    more (ValueError otherwise; teams of one are refused as they always were: they have no mates, plan them without teams=).  smooth= is the static smoother and stays a ValueError on a time plan.
    teams: a goal_rules.Teams: every plan is a TEAM plan, a time plan (layer_steps required, also in a static scene) in which the
    members of a team plan in index order around the walks of the members before them; reserve: the cells (Chebyshev) a walk
    reserves around itself, 0 .. 4 (None: ceil(separation / h), ValueError above 4).  Prioritised planning is incomplete: a
    later member boxed in by reservations comes back UNREACHABLE.  retries (0 .. 8; it belongs to teams, ValueError otherwise):
    up to that many reordering rounds -- a team with parked members (UNREACHABLE or UNCONVERGED) is planned again with those
    members first, and the round with the fewest parked members is the plan; 0 plans once, in index order.  Rounds repair a
    member that an earlier one boxed in.  They do not repair two mates whose start cells, or whose goal cells, are within
    `reserve` of each other (they fail in every order), an earlier member still does not know a later member's start cell, and
    only a chain of at most retries + 1 orders is tried, not every order.  retries > 0 with time_smooth is refused.  With time_smooth a
    team plan is smoothed too (a team plan is a time plan: no MovingHazards needed): max_leg, the actions of a leg at most (8; None:
    no cap; it belongs to teams, ValueError otherwise) -- a leg reserves all of its cells in every layer of its span, so long legs
    shut later members out, and a member whose start cell an earlier member's leg covers comes back UNREACHABLE.
    assign: None (robot i goes to goal i, as given), "sum" or "makespan" (it belongs to teams, ValueError otherwise): every plan first
    assigns the goals inside each team -- the minimum-total matching of members and goals, or the one that minimises the largest
    member cost first and then the total -- on each robot's own static cost-to-go (goal_rules.grid_assign), and plans the assigned
    goals.  A team that is already paired as well as any matching keeps its pairing.  The matching does not see reservations or
    the hazards' layers before the tail, teams are matched on their own, and a run is never reassigned.
    clearance: None, or (reach 1 .. 8, weight 1 .. 16): every plan pays weight * (reach + 1 - c) for entering a free cell whose
    Chebyshev distance c to the nearest blocked cell is at most reach, so paths keep away from obstacles where room exists
    (plan(..., clearance=) overrides it per call).  It belongs to static plans, plain or with smooth=: with moving hazards, teams=,
    time_smooth= or assign= it is a ValueError.  The plan is then no longer the shortest, a doorway narrower than 2 reach cells is
    still used (its surcharge is paid), `cost` includes the surcharges and `moves` stays the walk's length."""

    def __init__(self, env, walls=None, hazards=None, cells=64, inflate=None, max_waypoints=16, engine=None, extent=None,
                 smooth=False, los_margin=1, layer_steps=None, layers=None, teams=None, reserve=None, time_smooth=False, max_leg=_UNSET,
                 retries=0, assign=None, clearance=None):
        from .envs.vec_env import DeviceGoalVecEnv
        if teams is not None and not isinstance(teams, rules.Teams):
            raise TypeError(f"teams must be a mobrob_amd.envs.goal_rules.Teams, not {type(teams).__name__}")
        if teams is None and reserve is not None:
            raise ValueError("GridPlanner: reserve= belongs to teams=")
        if max_leg is not _UNSET and teams is None:
            raise ValueError("GridPlanner: max_leg= belongs to teams= with time_smooth (the cap on a smoothed team plan's legs)")
        if teams is None and not (isinstance(retries, (int, np.integer)) and not isinstance(retries, bool) and retries == 0):
            raise ValueError("GridPlanner: retries= belongs to teams= (reordering rounds of a team plan)")
        self.retries = rules.plan_retries_check(retries)
        if assign is not None:
            if teams is None:
                raise ValueError("GridPlanner: assign= belongs to teams= (goals are assigned inside a team)")
            rules.plan_assign_objective(assign)
        self.assign_objective = assign
        self.max_leg = 8 if max_leg is _UNSET else (None if max_leg is None else rules.plan_max_leg_check(max_leg))
        self.teams = teams
        self.timed = isinstance(hazards, rules.MovingHazards) or teams is not None
        if self.timed:
            if isinstance(hazards, rules.MovingHazards):
                rules.plan_scene_time(walls, hazards)
            else:
                rules.plan_scene(walls, hazards)
            if layer_steps is None:
                raise ValueError("GridPlanner: moving hazards and teams need layer_steps= (the steps a robot is given for one move)")
            if smooth:
                raise ValueError("GridPlanner: smooth=True with moving hazards or teams: smoothing over time is not supported by smooth= "
                                 "(a time plan takes time_smooth=True)")
            _, self.layer_steps, self.layers = rules.plan_time_check(0, layer_steps, 64 if layers is None else layers)
        else:
            rules.plan_scene(walls, hazards)
            if layer_steps is not None or layers is not None:
                raise ValueError("GridPlanner: layer_steps= and layers= belong to moving hazards (a goal_rules.MovingHazards)")
        self.walls, self.hazards, self.K = walls, hazards, int(max_waypoints)
        if self.K < 1:
            raise ValueError("max_waypoints must be >= 1")
        if isinstance(los_margin, bool) or los_margin not in (0, 1):
            raise ValueError(f"los_margin must be 0 or 1, got {los_margin!r}")
        self.smooth, self.los_margin = bool(smooth), int(los_margin)
        self.time_smooth = self._time_smooth_ok(time_smooth)
        self.clearance = self._clearance_ok(clearance)
        self.device = isinstance(env, DeviceGoalVecEnv)
        if self.device:
            self.engine = getattr(engine, "engine", engine)
            if self.engine is None:
                raise ValueError("GridPlanner on a DeviceGoalVecEnv needs engine= (the PPOEngine, or the PPO that owns one)")
            self.env, self.pos_dim, env_extent = env, env.pos_dim, env.extent
        else:
            from .envs.wrapper import EnvWrapper, TimeLimit, get_env
            if isinstance(env, str):
                env = get_env(env, terminate_on_goal=False)
            while isinstance(env, TimeLimit):
                env = env.env
            if not isinstance(env, EnvWrapper):
                raise TypeError(f"GridPlanner: env must be a DeviceGoalVecEnv, an EnvWrapper or an env name, not {type(env).__name__}")
            self.engine, self.env, self.pos_dim = None, env, len(env.get_pos())
            env_extent = getattr(env.env, "extent", None)
        if extent is None:
            extent = env_extent
        if extent is None:
            raise ValueError("GridPlanner: this environment has no extent; give extent=")
        if self.pos_dim not in (2, 3):
            raise ValueError(f"GridPlanner: the grid is x and y; the environment has {self.pos_dim} position dimension(s)")
        self.spec = rules.GridSpec(extent, cells, inflate)
        if teams is not None:
            self.reserve = rules.plan_team_reserve(teams, self.spec) if reserve is None else rules.plan_team_check(teams, reserve, teams.size)[1]
        self._kept = None        # the latest full plan: its goal cells, scenes and (device: resident, host: arrays) fields

    def _time_smooth_ok(self, time_smooth):
        """-> bool(time_smooth), or ValueError where it is asked for on a plan that is not a time plan (no moving hazards, no teams) or
        with teams of one: a team of one has no mate to plan around, so it stays refused as before (plan it without teams=)"""
        if time_smooth and self.retries > 0:
            raise ValueError("GridPlanner: retries > 0 with time_smooth=True is not supported (reordering rounds plan unsmoothed team plans only)")
        if time_smooth and (self.teams.size < 2 if self.teams is not None else not isinstance(self.hazards, rules.MovingHazards)):
            raise ValueError("GridPlanner: time_smooth=True needs hazards that are a MovingHazards and no teams, or teams of two or more (a team "
                             "of one has no mates: plan it without teams=; a static plan takes smooth=True)")
        return bool(time_smooth)

    def _clearance_ok(self, clearance):
        """-> None or the checked (reach, weight); ValueError naming `clearance` where it is asked for on a plan that is not static"""
        if clearance is None:
            return None
        for what, on in (("hazards=MovingHazards", isinstance(self.hazards, rules.MovingHazards)), ("teams=", self.teams is not None),
                         ("time_smooth=", self.time_smooth), ("assign=", self.assign_objective is not None)):
            if on:
                raise ValueError(f"GridPlanner: clearance= with {what} is not supported (surcharges belong to static plans, plain or smooth=)")
        return rules.plan_clearance_check(clearance)

    def _check(self, start, goal):
        start, goal = np.asarray(start, np.float64), np.asarray(goal, np.float64)
        if goal.ndim != 2 or goal.shape[1] != self.pos_dim or start.shape != goal.shape:
            raise ValueError(f"plan: start and goal must both be [n_robots, {self.pos_dim}], got shapes {start.shape} and {goal.shape}")
        if not (np.all(np.isfinite(start)) and np.all(np.isfinite(goal))):
            raise ValueError("plan: start and goal must be finite")
        for sc in (self.walls, self.hazards):
            if sc is not None:
                sc.check_robots(goal.shape[0])
        return start.astype(np.float32), goal.astype(np.float32)

    def _plan(self, start, goal, K, want_occupancy, want_fields, smooth=False, clearance=None):
        """One call.  The fields of the previous call are reused when this call's (scene, goal cell) list is the same.  smooth:
        the paths by line of sight -- on the device a first plan computes the fields with plan_grid and smooths on them, a round
        on unchanged goals runs k_plan_smooth alone.  clearance: (reach, weight) or None; the kept fields are reused only by a call
        with the same clearance (the engine keeps the two families resident side by side)."""
        _, scene = rules.plan_scene(self.walls, self.hazards)
        _, fcell, fscene = rules.plan_fields(self.spec, None, scene, goal)
        kept = self._kept
        same = kept is not None and np.array_equal(kept["field_goal_cell"], fcell) and np.array_equal(kept["field_scene"], fscene) and \
            kept.get("clearance") == clearance
        if self.device and clearance is not None:
            reuse = kept if same and not (want_occupancy or want_fields) and \
                kept["fields_id"] == getattr(self.engine, "_plan_clear_resident", None) else None
            if smooth and reuse is not None:
                out = dict(kept)
            else:
                out = self.engine.plan_grid_clear(self.spec, self.walls, self.hazards, clearance=clearance, start=start, goal=goal,
                                                  max_waypoints=K, want_occupancy=want_occupancy, want_fields=want_fields, reuse=reuse)
                self.engine._plan_clear_resident = out["fields_id"]
                if reuse is not None:
                    out["sweeps"] = kept["sweeps"]
            if smooth:
                out.update(self.engine.plan_smooth_clear(self.spec, reuse=out, start=start, goal=goal, scene=scene, max_waypoints=K,
                                                         margin=self.los_margin))
            out["fields_reused"] = reuse is not None
        elif self.device:
            reuse = kept if same and not (want_occupancy or want_fields) and kept["fields_id"] == getattr(self.engine, "_plan_resident", None) else None
            if smooth and reuse is not None:
                out = dict(kept)
            else:
                out = self.engine.plan_grid(self.spec, self.walls, self.hazards, start=start, goal=goal, max_waypoints=K,
                                            want_occupancy=want_occupancy, want_fields=want_fields, reuse=reuse)
                self.engine._plan_resident = out["fields_id"]
                if reuse is not None:
                    out["sweeps"] = kept["sweeps"]
            if smooth:
                out.update(self.engine.plan_smooth(self.spec, reuse=out, start=start, goal=goal, scene=scene, max_waypoints=K,
                                                   margin=self.los_margin))
            out["fields_reused"] = reuse is not None
        else:
            out = rules.grid_plan(self.spec, self.walls, self.hazards, start, goal, K, kept["occupancy"] if same else None,
                                  kept["fields"] if same else None, smooth=smooth, margin=self.los_margin, clearance=clearance)
            out["fields_reused"] = bool(same)
            if clearance is not None:
                out["clearance"] = clearance
        if not smooth:
            out.pop("moves", None)
        self._kept = out
        return out

    def _plan_time(self, start, goal, K, step0, want_occupancy, want_fields, smooth=False):
        """One time plan: the device call, or the NumPy rule on the host path.  smooth: over time"""
        if self.teams is not None:
            kw = dict(step0=step0, layer_steps=self.layer_steps, layers=self.layers)
            if smooth and self.device:
                return self.engine.plan_smooth_team(self.spec, self.walls, self.hazards, teams=self.teams, reserve=self.reserve, start=start,
                                                    goal=goal, max_waypoints=K, margin=self.los_margin, max_leg=self.max_leg,
                                                    want_occupancy=want_occupancy, want_fields=want_fields, **kw)
            if smooth:
                return rules.grid_plan_team(self.spec, self.walls, self.hazards, start, goal, K, self.teams, self.reserve, want_fields=want_fields,
                                            smooth=True, margin=self.los_margin, max_leg=self.max_leg, **kw)
            if self.retries > 0 and self.device:
                return self.engine.plan_grid_team_rounds(self.spec, self.walls, self.hazards, teams=self.teams, reserve=self.reserve,
                                                         retries=self.retries, start=start, goal=goal, max_waypoints=K,
                                                         want_occupancy=want_occupancy, want_fields=want_fields, **kw)
            if self.retries > 0:
                return rules.grid_plan_team_rounds(self.spec, self.walls, self.hazards, start, goal, K, self.teams, self.reserve,
                                                   want_fields=want_fields, retries=self.retries, **kw)
            if self.device:
                return self.engine.plan_grid_team(self.spec, self.walls, self.hazards, teams=self.teams, reserve=self.reserve, start=start,
                                                  goal=goal, max_waypoints=K, want_occupancy=want_occupancy, want_fields=want_fields, **kw)
            return rules.grid_plan_team(self.spec, self.walls, self.hazards, start, goal, K, self.teams, self.reserve, want_fields=want_fields, **kw)
        if self.device:
            kw = dict(start=start, goal=goal, step0=step0, layer_steps=self.layer_steps, layers=self.layers, max_waypoints=K,
                      want_occupancy=want_occupancy, want_fields=want_fields)
            if smooth:
                return self.engine.plan_smooth_time(self.spec, self.walls, self.hazards, margin=self.los_margin, **kw)
            return self.engine.plan_grid_time(self.spec, self.walls, self.hazards, **kw)
        return rules.grid_plan_time(self.spec, self.walls, self.hazards, start, goal, K, step0, self.layer_steps, self.layers,
                                    smooth=smooth, margin=self.los_margin)

    def assign(self, start, goal, step0=0, want_matrix=False):
        """The assignment on its own: start, goal [n][P] -> goal_rules.grid_assign's dict (assign, goal = goal[assign], assign_cost,
        assign_total, assign_max, assign_identity_total, assign_identity_max, assign_changed, assign_status, assign_potentials, and
        with want_matrix assign_matrix), by the device call on a DeviceGoalVecEnv and by the NumPy rule on the host path, as `plan`
        chooses.  The planner needs teams=; the objective is the planner's assign= ("sum" where that is None)."""
        if self.teams is None:
            raise ValueError("GridPlanner.assign: the planner has no teams= (goals are assigned inside a team)")
        start, goal = self._check(start, goal)
        kw = dict(objective=self.assign_objective or "sum", step0=step0, want_matrix=want_matrix)
        if isinstance(self.hazards, rules.MovingHazards):
            kw.update(layer_steps=self.layer_steps, layers=self.layers)
        if self.device:
            return self.engine.plan_assign(self.spec, self.walls, self.hazards, teams=self.teams, start=start, goal=goal, **kw)
        return rules.grid_assign(self.spec, self.walls, self.hazards, start, goal, self.teams, **kw)

    def plan(self, start, goal, step0=0, *, grow=False, want_occupancy=False, want_fields=False, smooth=None, time_smooth=None,
             clearance=_UNSET):
        """start, goal [n][P] -> dict: waypoints [n][K][P] float32 (z: the goal's), n_waypoints [n] (= min(count, K)), count [n]
        waypoints of the full path, status [n] (goal_rules.PLANNED 0, UNREACHABLE 1, TRUNCATED 2; UNCONVERGED 3: a device loop hit
        its bound), cost [n] int32 (-1: unreachable), cost_distance [n] float64 = cost * h / 5 (NaN: unreachable), field_of [n],
        field_goal_cell [F], field_scene [F]; with want_occupancy / want_fields also occupancy bool [S][G][G] / fields int32
        [F][G][G].  grow: when a robot's path was truncated, plan again with K = count.max() (this call only).  smooth: None (the
        planner's setting), True or False: line-of-sight smoothing with the planner's los_margin; `smoothed` tells which, `moves`
        [n] int32 is the number of moves of each robot's walk (None on an unsmoothed plan); `grow` then uses the smoothed count.
        With moving hazards the plan starts at the global step `step0` and the dict gains waits, leave [n][K], arrive [n] (waits at
        each waypoint's anchor, actions before the move that leaves it, actions of the walk), release [n][K] (the global step until
        which the robot holds at the anchor, 0: no hold) and `schedule`, a Schedule(release, home=start) for follow_waypoints;
        occupancy and fields then carry the layer axis, [S][T + 1][G][G] and [F][T + 1][G][G].  With teams the plan is such a time
        plan too (every robot has its own field; occupancy: the base layers) and gains team_clearance and team_crossings [n_teams]
        (goal_rules.grid_team_clearance of the planned walks: more than `reserve` cells and no crossing between planned mates).
        time_smooth: None (the planner's setting), True or False: smoothing over time with the planner's los_margin (and, with
        teams, max_leg; the dict then gains `keeps`, per robot the kept action indices in full, and team_clearance is
        goal_rules.grid_team_clearance_legs's: mates that keep to their legs stay more than `reserve` cells apart whatever their
        speeds).  `smoothed` is then True, `moves` [n] the moves of each walk, leave[k] the action index of waypoint k's
        anchor, release a hold at EVERY anchor but the start (goal_rules.grid_release_smooth), waits all zero; `grow` uses the
        smoothed count.  A kept leg of two or more actions is clear in every layer it spans; the count may exceed the unsmoothed
        plan's.  With the planner's retries > 0 a team plan is the best of its reordering rounds and the dict gains team_order
        [n_teams][size] (the order that plan was made in), team_rounds (rounds planned), team_parked and team_parked_first
        [n_teams] (members without a walk in that plan and in index order) (goal_rules.grid_plan_team_rounds).
        With the planner's assign= the goals are first assigned inside every team (`assign`), the plan is made for the assigned
        goals -- `grow` plans the same assignment again -- and the dict gains goal_rules.ASSIGN_KEYS: assign [n], goal [n][P] (the
        goals the plan was made for: hand THESE to `callback` and to the tracker), assign_cost [n], assign_total, assign_max,
        assign_identity_total, assign_identity_max, assign_changed and assign_status [n_teams].
        clearance: not given (the planner's setting), None or (reach, weight): the clearance-aware static plan, plain or smoothed;
        the dict then gains `clearance` and clearance_min [n] int32, the least clearance in cells (capped at reach + 1) over the
        cells each walk enters (-1: no walk); `cost` includes the surcharges paid, `fields` are the cost fields."""
        clearance = self.clearance if clearance is _UNSET else self._clearance_ok(clearance)
        start, goal = self._check(start, goal)
        assigned = None
        if self.assign_objective is not None:
            assigned = self.assign(start, goal, step0)
            goal = np.ascontiguousarray(assigned["goal"], np.float32)
        smooth = self.smooth if smooth is None else bool(smooth)
        time_smooth = self.time_smooth if time_smooth is None else self._time_smooth_ok(time_smooth)
        if clearance is not None and time_smooth:
            raise ValueError("plan: clearance= with time_smooth= is not supported (surcharges belong to static plans, plain or smooth=)")
        if self.timed:
            if smooth:
                raise ValueError("plan: smooth=True with moving hazards or teams: smoothing over time is not supported by smooth= "
                                 "(a time plan takes time_smooth=True)")
            out = self._plan_time(start, goal, self.K, step0, want_occupancy, want_fields, time_smooth)
            if grow and np.any(out["status"] == rules.TRUNCATED):
                out = self._plan_time(start, goal, int(out["count"].max()), step0, want_occupancy, want_fields, time_smooth)
            out["fields_reused"] = False
            smooth = time_smooth
        else:
            if step0 != 0:
                raise ValueError("plan: step0 belongs to moving hazards; a static plan has no clock")
            out = self._plan(start, goal, self.K, want_occupancy, want_fields, smooth, clearance)
            if grow and np.any(out["status"] == rules.TRUNCATED):
                out = self._plan(start, goal, int(out["count"].max()), want_occupancy, want_fields, smooth, clearance)
        res = {k: out[k] for k in ("waypoints", "n_waypoints", "count", "status", "cost", "field_of", "field_goal_cell", "field_scene",
                                   "fields_reused")}
        if self.timed:
            res.update({k: out[k] for k in ("waits", "leave", "arrive", "release")})
            res["schedule"] = rules.Schedule(out["release"], home=start)
        if self.teams is not None:
            res.update({k: out[k] for k in ("team_clearance", "team_crossings")})
            if "keeps" in out:
                res["keeps"] = out["keeps"]
            if self.retries > 0:
                res.update({k: out[k] for k in rules.TEAM_ROUND_KEYS})
        if assigned is not None:
            res.update({k: assigned[k] for k in rules.ASSIGN_KEYS})
        if clearance is not None:
            res["clearance"], res["clearance_min"] = clearance, out["clearance_min"]
        res["cost_distance"] = np.where(out["cost"] >= 0, out["cost"].astype(np.float64) * float(self.spec.h) / rules.PLAN_STEP, np.nan)
        res["smoothed"], res["moves"] = smooth, out.get("moves")
        if want_occupancy:
            res["occupancy"] = out["occupancy"]
        if want_fields:
            res["fields"] = out["fields"]
        if out.get("sweeps") is not None:
            res["sweeps"] = out["sweeps"]
        return res

    def plan_spec(self, start, spec, goal=None, pace=None, max_waypoints=None, *, state=None, step0=0, partial=False, share=None,
                  objective="makespan"):
        """A plan from a specification: the avoid clauses of `spec` (Spec.always(outside(...)) over the whole run)
        become obstacles beside the planner's walls and hazards, its reach clauses (Spec.eventually / Spec.stay over inside(...),
        at most 8) stations, and per robot the order of the stations is chosen -- the shortest tour that keeps every window and
        dwell -- and the waypoints stitched, all robots in one call: the device call on a DeviceGoalVecEnv, the NumPy rule on the
        host path (goal_rules.spec_plan; device: mobrob_ppo_spec_plan), bit for bit.  start [n][P]; goal [n][P] or None: where
        the robots end after the last station; pace: the steps a robot is given for one orthogonal move (an integer >= 1; None: 1
        where no station has a window or a dwell, a ValueError naming pace= where one has); max_waypoints: the K slots (None: the
        planner's).  Returns goal_rules.spec_plan's dict (waypoints, n_waypoints, count, status, cost in ticks, tour_order, tour_eta,
        station_waypoint, release, station_cell, station_margin, covered, matrix, ...) and `schedule`: a
        Schedule(release, home=start) for follow_waypoints where any release is nonzero, else None.
        Refused by name: a planner with teams=, moving hazards, clearance= or smooth= (legs are not smoothed, teams and moving
        hazards are not planned from a specification), and everything goal_rules.spec_plan_parse refuses of the specification.
        pace is an estimate of the policy's speed: a robot that arrives later than planned dwells for less time, and the monitor
        after the run remains the judge.
        From the middle of a run (goal_rules.spec_plan's state=, step0=, partial=; device: mobrob_ppo_spec_replan): state is the
        monitor's SpecState, or the run's FollowState, whose .spec and .step0 are then taken (a step0= that disagrees is refused,
        as is a FollowState of a run without a specification); the stations whose clause is already satisfied are left out, the
        plan starts at step0, and with partial=True a robot keeps the stations it can still keep.  The dict then also holds
        tour_len, dropped and done (SPEC_REPLAN_KEYS).  A dwell in progress earns no credit: the robot dwells again in full.
        A team shares the stations (goal_rules.spec_plan's share=, objective=; device: mobrob_ppo_spec_plan_share):
        share is the team size (consecutive robots, as Teams), and each station the team still has to visit goes to one member --
        the smallest makespan, then the smallest sum of the members' costs, or with objective="sum" the smallest sum.  The dict then
        also holds share, team_cover, team_dropped, team_makespan, team_total and team_done (SPEC_SHARE_KEYS).  The planner itself
        still has no teams=: mates do not plan around each other on their tours."""
        from .waypoints import FollowState
        if isinstance(state, FollowState):
            if state.spec is None:
                raise ValueError("plan_spec: state is a FollowState of a run without a specification (follow_waypoints(..., spec=))")
            if step0 not in (0, state.step0):
                raise ValueError(f"plan_spec: step0 = {step0} disagrees with the FollowState's step0 = {state.step0}")
            state, step0 = state.spec, int(state.step0)
        for what, on in (("teams=", self.teams is not None), ("hazards=MovingHazards", isinstance(self.hazards, rules.MovingHazards)),
                         ("clearance=", self.clearance is not None), ("smooth=", self.smooth), ("time_smooth=", self.time_smooth)):
            if on:
                raise ValueError(f"GridPlanner.plan_spec: a planner with {what} is not supported (a plan from a specification is the "
                                 "static, unsmoothed plan of single robots)")
        K = self.K if max_waypoints is None else int(max_waypoints)
        start = np.asarray(start, np.float64)
        if start.ndim != 2 or start.shape[1] != self.pos_dim:
            raise ValueError(f"plan_spec: start must be [n_robots, {self.pos_dim}], got shape {start.shape}")
        if self.device:
            out = self.engine.plan_spec(self.spec, self.walls, self.hazards, spec=spec, start=start, goal=goal, pace=pace, max_waypoints=K,
                                        state=state, step0=step0, partial=partial, share=share, objective=objective)
        else:
            out = rules.spec_plan(self.spec, self.walls, self.hazards, spec, start, goal, K, pace, state=state, step0=step0, partial=partial,
                                  share=share, objective=objective)
        out["schedule"] = rules.Schedule(out["release"], home=start) if np.any(out["release"] != 0) else None
        return out

    def spec_callback(self, spec, goal=None, pace=None, partial=True, when="stalled", share=None, objective="makespan"):
        """The planner of waypoints.follow_with_replanning for a run that follows a plan from a specification: its attribute
        `wants_state` is True, so the loop calls it as planner(positions, status, reached, state=the run's FollowState), and it
        plans again with plan_spec(positions, spec, goal, pace, state=state, partial=partial): the stations the monitor has seen
        satisfied are left out and the plan starts at the run's step.  when="stalled": the STALLED robots are replanned;
        when="all": every robot that is not FINISHED.  A chosen robot whose new plan is PLANNED with count > 0 gets
        (waypoints[:count], release[:count]) -- so the run needs a schedule from its first call --; the others are left alone.
        `callback.last` holds the latest plan (None before the first, and after a call without a robot to replan the plan of the
        call before), `callback.calls` counts the calls.  The monitor is read, never written.
        share= (a team size) and objective=: the plan is plan_spec(..., share=, objective=), and a team with any chosen member is
        replanned as a whole: every member that is not FINISHED and whose new plan is PLANNED with count > 0 gets its tuple."""
        from .waypoints import FINISHED, STALLED
        if when not in ("stalled", "all"):
            raise ValueError(f"spec_callback: when must be 'stalled' or 'all', got {when!r}")
        rules.spec_plan_parse(spec)
        if share is not None:
            share, objective = rules.spec_plan_share_size(share, objective)     # the robots are counted when the plan is made

        def planner(positions, status, reached, state=None):
            planner.calls += 1
            if state is None:
                raise ValueError("spec_callback: the planner needs the run's state (follow_with_replanning hands it to a planner "
                                 "whose wants_state is true)")
            status = np.asarray(status)
            chosen = np.nonzero(status == STALLED if when == "stalled" else status != FINISHED)[0]
            if chosen.size == 0:
                return {}
            plan = self.plan_spec(positions, spec, goal=goal, pace=pace, state=state, partial=partial, share=share, objective=objective)
            planner.last = plan
            if share is not None:                          # the whole team of a chosen robot, its finished members aside
                mates = np.unique(chosen // share)[:, None] * share + np.arange(share)
                chosen = np.array([i for i in mates.ravel() if status[i] != FINISHED], np.int64)
            return {int(i): (plan["waypoints"][i, :plan["count"][i]].copy(), plan["release"][i, :plan["count"][i]].copy())
                    for i in chosen if plan["status"][i] == rules.PLANNED and plan["count"][i] > 0}
        planner.last, planner.calls, planner.wants_state = None, 0, True
        return planner

    def callback(self, goal, horizon=None):
        """The `planner(positions, status, reached)` of waypoints.follow_with_replanning for the goals `goal` [n][P]: every
        STALLED robot is planned again from where it stands -- all robots in one call, so the fields of the unchanged goals are
        reused and only the paths are walked -- and gets {robot: waypoints[:count]}; robots whose plan is not PLANNED (unreachable
        from there, or longer than max_waypoints) are left alone.  The plans are smoothed when the planner is (`smooth=`).
        `callback.last` holds the latest plan (None before the first).
        With moving hazards `horizon` is required, the `horizon` of that follow_with_replanning loop: the loop makes call r of the
        callback after r * horizon steps, so the callback counts its own calls (`callback.calls`) and plans with step0 = r * horizon;
        a robot then gets (waypoints[:count], release[:count]), which the loop hands to FollowState.replan(..., release=).  The
        plans are smoothed over time when the planner is (`time_smooth=`); the tuples are the same.
        With teams (horizon required as well) a team with any STALLED member is planned again as a whole from where its members
        stand: every member that is not FINISHED and whose new plan is PLANNED gets (waypoints, release); finished members are
        planned too, so that they reserve their cell, and are not returned.
        The callback NEVER reassigns: with the planner's assign= hand it plan["goal"], the goals the first plan was made for; it
        plans to the goals as given, robot i to goal[i]."""
        from .waypoints import FINISHED, STALLED
        goal = np.asarray(goal, np.float64)
        if self.timed:
            if isinstance(horizon, bool) or not isinstance(horizon, (int, np.integer)) or horizon < 1:
                raise ValueError(f"callback: moving hazards and teams need horizon= (the replanning loop's, an integer >= 1), got {horizon!r}")
        elif horizon is not None:
            raise ValueError("callback: horizon= belongs to moving hazards; a static plan has no clock")

        def planner(positions, status, reached):
            planner.calls += 1
            stalled = np.nonzero(np.asarray(status) == STALLED)[0]
            if stalled.size == 0:
                return {}
            objective, self.assign_objective = self.assign_objective, None     # the goals as given: a run is never reassigned
            try:
                plan = self.plan(positions, goal, planner.calls * int(horizon)) if self.timed else self.plan(positions, goal)
            finally:
                self.assign_objective = objective
            planner.last = plan
            if self.teams is not None:                     # the whole team of a stalled robot, its finished members aside
                mates = np.unique(stalled // self.teams.size)[:, None] * self.teams.size + np.arange(self.teams.size)
                stalled = np.array([i for i in mates.ravel() if np.asarray(status)[i] != FINISHED], np.int64)
            rows = {int(i): plan["waypoints"][i, :plan["n_waypoints"][i]].copy() for i in stalled if plan["status"][i] == rules.PLANNED}
            if self.timed:
                rows = {i: (w, plan["release"][i, :len(w)].copy()) for i, w in rows.items()}
            return rows
        planner.last, planner.calls = None, 0
        return planner
