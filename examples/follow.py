#!/usr/bin/env python3
"""Drive a trained goal-conditioned policy along a planner's waypoints and report whether, and when, the robots get there.

    python examples/follow.py --env-name point --policy-name ppo --waypoints path.npy --robots 4096

`--waypoints FILE.npy` holds `[K][P]` positions (the same path for every robot) or `[n][K][P]` (one path per robot, n = --robots).
Each robot starts at rest at a position drawn from the environment's start region (`--seed`) and follows its waypoints in
order: a waypoint counts as reached after the step that ends inside the reach radius, and the next one becomes the goal
(mobrob_amd.waypoints).  The checkpoint is loaded as examples/control.py loads it (data/policies/<env>-<policy>.zip).

By default all robots run in ONE device call (DeviceGoalVecEnv, the kinematic stand-in stepped by the engine); `--host` runs
the same semantics as a Python loop over `get_env(...)` with one `predict` per robot and step.  Three report lines: the success
rate (all waypoints reached), the mean number of waypoints reached, and the mean arrival step of the last waypoint over the
robots that reached it (nan if none did).

`--hazards FILE.npy` ([M][2] hazard centres; `--hazard-size R`, default 0.3) adds the reference Engine's hazard cost (shaped,
coefficient 1) and three more lines: the mean cost per robot, the violation rate (robots that entered a hazard) and the minimum
clearance (distance to the nearest hazard boundary) over all robots and steps.

`--hazard-frames FILE.npy` ([F][M][3]: x, y, radius of M hazards in F frames) makes the hazards move instead: frame
min(g // N, F - 1) is in force at step g with `--frame-steps N` (default 1), frame (g // N) % F with `--hazard-loop`.  It
replaces --hazards / --hazard-size, reports the same three lines and works with --horizon / --leg-steps (g is the run's step).

`--horizon H` runs the same job the way a planner would drive it: a chain of calls of H steps each (the last one shorter if H
does not divide --max-steps), every call continuing from the state the previous one returned.  The report is exactly the single
call's.  `--leg-steps B` gives every waypoint a budget of B steps: a robot that has spent it without arriving stalls (and would
be the planner's to replan); a fourth line then reports the rate of stalled robots.

`--release FILE.npy` ([K] or [n][K] integers) times the waypoints: waypoint k may not become a robot's goal before the global step
release[k]; until then the robot holds at the previous waypoint (its start for k = 0) under the policy.  `--stagger S` is the
shorthand for delays: robot m of a team (robot i without --team-size) gets every waypoint released m * S steps later.  Two lines
report the mean hold steps per robot and the largest drift from an anchor while holding.  With --team-size, a stagger of the
time a robot needs to clear a crossing is the one-line demonstration that delays remove team conflicts.

`--walls FILE.npy` ([M][4]: centre x, y and half extents hx, hy of M axis-aligned boxes) checks every step against walls:
contact of the robot's footprint (`--robot-radius R`, default 0.1) and crossing of the step's segment, which also sees a step that
jumps a thin wall.  `--arena` adds the reference's turtlebot3 enclosure (four boxes, 2.98 m outside, 0.265 m thick).  Three lines
report the contact rate, the crossing rate (robots with such a step) and the minimum clearance to a wall.  Walls block nothing unless `--solid` is given: robots then stop and slide at them.  Team-mates block nothing unless `--team-solid` is given (with --team-size): a robot then stops or slides at the square of half-width --separation around each mate, the lower team index first, and three lines report the blocked rate, the stopped steps and the steps inside a mate's square
(goal_rules.wall_block), and two more lines report the share of robots blocked at least once and the fully stopped steps.

`--goal X,Y` (X,Y,Z for a drone) PLANS the waypoints instead of reading them: a grid of `--plan-cells` (32, 64, 128; default 64)
cells a side over the arena, blocked where --walls / --arena / --hazards are (mobrob_amd.planning.GridPlanner), one path per robot
from its start to the goal.  It excludes --waypoints.  A first line reports the rate of robots with a plan; the others count a
robot without one as not successful.  With --horizon and --leg-steps a stalled robot is planned again from where it stands between
the calls (the planner's callback).  With `--hazard-frames` the plan is made over TIME: a robot is given `--plan-layer-steps` steps
(default 10) for one move or wait, `--plan-layers` (default 64) of them are planned against the frames in force, and where the
cheapest plan waits for a hazard to pass the run gets the release steps as its schedule (so --release / --stagger and
--plan-smooth are excluded).  `--plan-time-smooth` (with --hazard-frames or --team-size) smooths such a plan over time: a
straight leg is kept only where it is clear, at --plan-los-margin, in every layer it spans, and the schedule holds the robot at
every anchor until the leg's first layer.  With `--team-size` the mates of a team are planned around each other the same way (a time plan, also
in a static scene): `--plan-reserve` cells are kept around every planned walk, and a line reports the smallest planned team
clearance beside the run's measured conflicts; with `--plan-time-smooth` a team plan's legs are at most `--plan-max-leg` actions long
(default 8, 0: no cap) and every leg is reserved whole for the mates that plan later; `--plan-retries R` (0 .. 8, default 0) plans
a team whose members stayed parked again, up to R times, with those members first, and a line reports the parked members before
and after.  `--plan-smooth` smooths every plan by line
of sight (fewer waypoints: only the cells a straight leg cannot skip), `--plan-los-margin` (0 or 1, default 1) is the clearance of
that test in cells; a second line then reports the waypoints and the moves per planned robot.  `--plan-clearance REACH,WEIGHT`
(a static plan only: it excludes --hazard-frames, --team-size and --plan-time-smooth) makes the plan pay WEIGHT * (REACH + 1 - c) for
entering a cell c <= REACH cells from a blocked one, so it keeps away from obstacles where room exists; a line reports the
waypoints per planned robot and the least clearance of the walks beside those of the plan without it.

`--goals FILE.npy` plans to a SET of places instead of one goal: `[size][P]` (the places of one team, the same for every team;
size = --team-size) or `[n][P]` (one per robot).  It excludes --goal and --waypoints.  As given, robot i is planned to goals[i];
`--assign sum` or `--assign makespan` (it needs --team-size) first assigns the places inside every team -- the pairing of least
total path cost, or the one whose longest path is shortest -- and a line reports the teams whose pairing changed and the total
before and after (mobrob_amd.planning.GridPlanner(assign=)).  A run is never reassigned: replanning keeps the assigned goals.

`--check-spec --plan-spec [--pace N]` lets the specification that --check-spec monitors drive the plan: its stations (here the reach
circle around --goal; with --spec-hold H a stay of H steps, which needs --pace, the steps a robot is given for one orthogonal move)
are planned with GridPlanner.plan_spec in place of the plan to --goal, the walls once more as keep-out regions; the run follows the
plan's schedule, the monitor then judges it.  It excludes --hazard-frames, --team-size, --plan-smooth and --plan-clearance.
`--replan-spec` (with --plan-spec, --horizon and --leg-steps) plans a stalled robot again between the calls of the run, from where it
stands and at the run's step, for the stations the monitor has not seen satisfied yet (GridPlanner.spec_callback); `--partial` lets
a robot that cannot keep every window keep the stations it still can, in the first plan and in every later one.
`--share N [--share-objective sum]` (with --plan-spec; it excludes --team-size) shares the stations within teams of N consecutive
robots: each station is visited by one member (plan_spec(share=N): the team done as early as possible, or with the least total), the
others get no tour, and after the run the team's verdict is printed beside the robots' (waypoints.spec_team_result: someone reached).
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def check_chain(max_steps, horizon, leg_steps):
    """-> the step counts of the chain's calls (one call without --horizon); ValueError for arguments no run can have"""
    max_steps, leg_steps = int(max_steps), int(leg_steps)
    if max_steps < 1:
        raise ValueError("--max-steps must be >= 1")
    if leg_steps < 0:
        raise ValueError("--leg-steps must be >= 0 (0: no budget)")
    if horizon is None:
        return [max_steps]
    horizon = int(horizon)
    if horizon < 1:
        raise ValueError("--horizon must be >= 1")
    return [min(horizon, max_steps - s) for s in range(0, max_steps, horizon)]


def follow(env_name, policy_name, waypoints, robots, max_steps=1000, host=False, seed=0, policy=None, hazards=None,
           horizon=None, leg_steps=0, hazard_frames=None, frame_steps=1, hazard_loop=False, team_size=None, separation=0.3,
           release=None, stagger=0, walls=None, arena=False, robot_radius=0.1, goal=None, plan_cells=64,
           plan_smooth=False, plan_los_margin=1, plan_layer_steps=10, plan_layers=64, plan_reserve=None, plan_time_smooth=False, plan_max_leg=None,
           plan_retries=0, goals=None, assign=None, plan_clearance=None, solid=False, tile256=False,
           tile256_wide=False, team_solid=False, check_spec=False, spec_hold=0, plan_spec=False, pace=None,
           replan_spec=False, partial=False, share=None, share_objective=None):
    if share is not None and not plan_spec:
        raise ValueError("--share needs --plan-spec (the plan whose stations the team shares)")
    if share is not None and team_size is not None:
        raise ValueError("--share excludes --team-size (mates do not plan around each other in a plan from a specification)")
    if share_objective is not None and share is None:
        raise ValueError("--share-objective needs --share")
    shared = {} if share is None else dict(share=int(share), objective=share_objective or "makespan")
    if check_spec and goal is None:
        raise ValueError("--check-spec needs --goal (the specification is: eventually inside the reach radius around the goal)")
    if int(spec_hold) != 0 and not check_spec:
        raise ValueError("--spec-hold needs --check-spec")
    if plan_spec and not check_spec:
        raise ValueError("--plan-spec needs --check-spec (the specification whose stations are planned)")
    if pace is not None and not plan_spec:
        raise ValueError("--pace needs --plan-spec")
    if replan_spec and not plan_spec:
        raise ValueError("--replan-spec needs --plan-spec (the plan that is made again during the run)")
    if partial and not plan_spec:
        raise ValueError("--partial needs --plan-spec")
    if team_solid and team_size is None:
        raise ValueError("--team-solid needs --team-size")
    if solid and walls is None and not arena:
        raise ValueError("--solid needs --walls or --arena")
    calls = check_chain(max_steps, horizon, leg_steps)
    if goals is not None and (goal is not None or waypoints is not None):
        raise ValueError("--goals excludes --goal and --waypoints")
    if assign is not None and (goals is None or team_size is None):
        raise ValueError("--assign needs --goals and --team-size (places are assigned inside a team)")
    if goals is None and (goal is None) == (waypoints is None):
        raise ValueError("give --waypoints or --goal, not both")
    from mobrob_amd import load_policy
    from mobrob_amd.envs.vec_env import DeviceGoalVecEnv
    from mobrob_amd.envs.goal_rules import Hazards, MovingHazards, Schedule, Teams, Walls
    from mobrob_amd.envs.wrapper import ROBOT_DIMS, KinematicSim
    from mobrob_amd.waypoints import follow_waypoints
    policy = load_policy(env_name, policy_name) if policy is None else policy
    if tile256 or tile256_wide:   # a 2x256 tanh policy: calls without hazards, teams or walls run as one launch (ValueError on any other policy)
        getattr(policy, "engine", policy).set_eval_tile256(True)
    if tile256_wide:   # ... and calls with hazards too (implies tile256); walls and teams stay on the per-step path
        getattr(policy, "engine", policy).set_eval_tile256_wide(True)
    d, a, p = ROBOT_DIMS[env_name]
    extent = KinematicSim(d, a, p).extent
    start = np.random.default_rng(seed).uniform(-extent / 2, extent / 2, (int(robots), p))   # the env's init_space
    env = env_name if host else DeviceGoalVecEnv.for_robot(env_name, int(robots), time_limit=0, seed=seed)
    hz = None if hazards is None else Hazards(hazards[0], hazards[1], indicator=False)
    if hazard_frames is not None:
        if hazards is not None:
            raise ValueError("--hazards and --hazard-frames exclude each other")
        fr = np.asarray(hazard_frames, np.float64)
        if fr.ndim != 3 or fr.shape[2] != 3:
            raise ValueError(f"--hazard-frames must hold [F][M][3] (x, y, radius), got shape {fr.shape}")
        hz = MovingHazards(fr[:, :, :2], fr[None, :, :, 2], frame_steps=int(frame_steps), loop=bool(hazard_loop), indicator=False)
    teams = None if team_size is None else Teams(int(team_size), float(separation), solid=bool(team_solid))   # (a ValueError names what is wrong)
    wl = None
    if walls is not None or arena:
        boxes = np.zeros((0, 4)) if walls is None else np.asarray(walls, np.float64)
        if boxes.ndim != 2 or boxes.shape[1] != 4:
            raise ValueError(f"--walls must hold [M][4] (cx, cy, hx, hy), got shape {boxes.shape}")
        wl = Walls(np.concatenate([boxes, Walls.enclosure()]) if arena else boxes, radius=float(robot_radius), indicator=False, solid=bool(solid))
    n_waypoints = replan = None
    if goals is not None:
        goals = np.asarray(goals, np.float64)
        rows = (int(robots),) if team_size is None else (int(team_size), int(robots))
        if goals.ndim != 2 or goals.shape[1] != p or p < 2 or goals.shape[0] not in rows or int(robots) % goals.shape[0]:
            raise ValueError(f"--goals must hold [team size][{p}] or [{int(robots)}][{p}] positions of robots that move in x and y, got shape {goals.shape}")
        goals = np.tile(goals, (int(robots) // goals.shape[0], 1))
        goal = goals[0]                                    # (from here on: "the waypoints are planned")
    def monitored_spec():   # eventually inside the reach circle around the goal (--spec-hold H: for H steps in a row); with walls: always outside every one;
        # with moving hazards: outside every one from the first step on; with teams: always further than the separation from every mate
        from mobrob_amd.envs.goal_rules import REACH_RADIUS, Regions, Spec, inside, outside
        boxes = np.zeros((0, 4), np.float32) if wl is None else wl.rows(0)
        regions = Regions(np.concatenate([[[goal[0], goal[1], REACH_RADIUS, 0.0]], boxes]), [1] + [0] * len(boxes))
        reach = Spec.eventually(inside(0)) if int(spec_hold) == 0 else Spec.stay(inside(0), int(spec_hold))   # (ValueError above SPEC_HOLD_MAX)
        clauses = [reach] + ([Spec.always(outside(1, 1 + len(boxes)))] if len(boxes) else [])
        if isinstance(hz, MovingHazards):   # --hazard-frames: never inside a moving hazard, from the first step on
            from mobrob_amd.envs.goal_rules import MovingRegions
            first = regions.max_regions
            regions = MovingRegions.join(regions, MovingRegions.from_hazards(hz))
            clauses.append(Spec.always(outside(first, regions.max_regions), a=1))
        if teams is not None:               # --team-size / --separation: always further than the separation from every mate
            from mobrob_amd.envs.goal_rules import apart
            clauses.append(Spec.always(apart(teams.separation)))
        return dict(spec=Spec(regions, clauses, team_size=1 if teams is None else teams.size), path_stride=1)
    if goal is not None:
        from mobrob_amd.planning import GridPlanner
        goal = np.asarray(goal, np.float64).reshape(-1)
        if goal.shape != (p,) or p < 2:
            raise ValueError(f"--goal must hold {p} coordinates of a robot that moves in x and y, got {goal.size}")
        if goals is None:
            goals = np.tile(goal, (int(robots), 1))
        timed = isinstance(hz, MovingHazards) or teams is not None     # with teams the mates are planned around each other, over time
        if timed and (release is not None or stagger):
            raise ValueError("--release / --stagger exclude --goal with --hazard-frames or --team-size: the time plan makes the schedule")
        planner = GridPlanner(env, walls=wl, hazards=hz, cells=int(plan_cells), engine=policy, smooth=bool(plan_smooth),
                              los_margin=int(plan_los_margin), time_smooth=bool(plan_time_smooth),
                              **(dict(max_leg=None if int(plan_max_leg) == 0 else int(plan_max_leg)) if plan_max_leg is not None else {}),
                              **(dict(layer_steps=int(plan_layer_steps), layers=int(plan_layers)) if timed else {}),
                              **(dict(teams=teams, reserve=None if plan_reserve is None else int(plan_reserve)) if teams is not None else {}),
                              **(dict(retries=int(plan_retries)) if int(plan_retries) != 0 else {}),
                              **(dict(assign=assign) if assign is not None else {}),
                              **(dict(clearance=tuple(plan_clearance)) if plan_clearance is not None else {}))
        if plan_clearance is not None:                     # the plan without it, made first: the run's plan stays the planner's latest
            from mobrob_amd.envs.goal_rules import grid_plan_clearance_min
            plain = planner.plan(start, goals, grow=True, clearance=None, want_occupancy=True, want_fields=True)
            plain_min = grid_plan_clearance_min(planner.spec, plain, start, goals, planner.clearance[0])
        if plan_spec:                                      # the specification's stations in --goal's place, in the order the plan chooses
            plan = planner.plan_spec(start, monitored_spec()["spec"], pace=pace, partial=bool(partial), **shared)
            plan.update(smoothed=False, moves=None)
            if shared:
                ok = plan["team_feasible"]
                print(f"shared within teams of {shared['share']} ({shared['objective']}): {int(ok.sum())} of {len(ok)} teams allotted, "
                      f"{int(np.sum(plan['share'] != 0))} members with stations, mean makespan "
                      f"{float(np.mean(plan['team_makespan'][ok])) if np.any(ok) else float('nan')} ticks")
            if replan_spec and plan["schedule"] is None:   # the replanned rows may bring release steps: the run has a schedule from its first call
                plan["schedule"] = Schedule(plan["release"], home=start)
            print(f"planned from the specification: tour cost {float(np.mean(plan['cost'][plan['status'] == 0])) if np.any(plan['status'] == 0) else float('nan')} "
                  f"ticks, {int(np.sum(plan['release'] != 0))} holds, stations covered: {bool(np.all(plan['covered']))}")
        else:
            plan = planner.plan(start, goals, grow=True)
        if plan_clearance is not None:
            ok, pk = plan["status"] == 0, plain["status"] == 0
            if np.any(ok) and np.any(pk):
                print(f"clearance plan {planner.clearance}: {float(np.mean(plan['count'][ok]))} waypoints per planned robot, least clearance "
                      f"{int(plan['clearance_min'][ok].min())} cells; without it: {float(np.mean(plain['count'][pk]))} waypoints, least "
                      f"clearance {int(plain_min[pk].min())} cells")
        if assign is not None:
            goals = plan["goal"]                           # the callback plans to the goals it is given and never reassigns
            print(f"assigned ({assign}): {int(plan['assign_changed'].sum())} of {len(plan['assign_changed'])} teams changed, total path cost "
                  f"{int(plan['assign_identity_total'].sum())} -> {int(plan['assign_total'].sum())}")
        waypoints, n_waypoints, plan_schedule = plan["waypoints"], plan["n_waypoints"], plan.get("schedule")
        replan = planner.callback(goals, **(dict(horizon=calls[0]) if timed else {})) if int(leg_steps) > 0 and not plan_spec else None
        if replan_spec:                                    # a stalled robot gets the stations it has not visited yet, from where it stands
            replan = planner.spec_callback(monitored_spec()["spec"], pace=pace, partial=bool(partial), **shared)
        print(f"planned rate: {float(np.mean(plan['status'] == 0))}")
        if teams is not None:                              # beside the run's measured team conflict steps, further down
            print(f"planned team clearance: {int(plan['team_clearance'].min())} cells at the least (reserve {planner.reserve}), "
                  f"{int(plan['team_crossings'].sum())} crossings")
        if "team_parked" in plan:
            print(f"planned with retries: {int(plan['team_parked_first'].sum())} parked members in index order, {int(plan['team_parked'].sum())} "
                  f"after at most {int(plan['team_rounds'].max())} rounds a team")
        if plan["smoothed"] and np.any(plan["status"] == 0):
            ok = plan["status"] == 0
            print(f"smoothed plan: {float(np.mean(plan['count'][ok]))} waypoints for {float(np.mean(plan['moves'][ok]))} moves per planned robot")
    schedule = make_schedule(release, stagger, int(robots), np.shape(waypoints)[-2], team_size)
    if goal is not None and plan_schedule is not None:
        schedule = plan_schedule
    monitored = monitored_spec() if check_spec else {}
    r = follow_waypoints(policy, env, start, waypoints, n_waypoints, max_steps=calls[0], deterministic=True, seed=seed, hazards=hz,
                         leg_steps=leg_steps, teams=teams, schedule=schedule, walls=wl, **monitored)
    for steps in calls[1:]:                                # the run, continued call after call
        if replan is not None:                             # a stalled robot is planned again from where it stands
            more = dict(state=r["state"]) if getattr(replan, "wants_state", False) else {}
            for robot, w in replan(np.array(r["state"].positions), r["status"], r["reached"], **more).items():
                if isinstance(w, tuple):                   # a time plan: the waypoints and their release steps
                    r["state"].replan([robot], np.asarray(w[0], np.float64)[None], release=w[1][None])
                else:
                    r["state"].replan([robot], np.asarray(w, np.float64)[None])
        r = follow_waypoints(policy, env, max_steps=steps, deterministic=True, seed=seed, hazards=hz, state=r["state"],
                             leg_steps=leg_steps, teams=teams, schedule=schedule, walls=wl, **monitored)
    K = r["arrival"].shape[1]
    done = r["reached"] == (K if goal is None else np.where(r["state"].n_waypoints > 0, r["state"].n_waypoints, -1))
    last = r["arrival"][done, (K if goal is None else r["state"].n_waypoints[done]) - 1]
    print(f"success rate: {float(np.mean(done))}")
    print(f"mean waypoints reached: {float(np.mean(r['reached']))}")
    print(f"mean arrival step of the last waypoint: {float(np.mean(last)) if last.size else float('nan')}")
    if int(leg_steps) > 0:
        print(f"stalled rate: {float(np.mean(r['status'] == 2))}")
    if hz is not None:
        report_hazards(r)
    if teams is not None:
        report_teams(r)
    if schedule is not None:
        print(f"mean hold steps: {float(np.mean(r['hold_steps']))}")
        print(f"maximum hold drift: {float(np.nanmax(r['hold_drift'])) if np.any(r['hold_steps'] > 0) else float('nan')}")
    if wl is not None:
        clear = r["min_wall_clearance"]
        print(f"wall contact rate: {float(np.mean(r['contact_steps'] > 0))}")
        print(f"wall crossing rate: {float(np.mean(r['crossing_steps'] > 0))}")
        if solid:
            print(f"wall blocked rate: {float(np.mean(r['wall_blocked_steps'] > 0))}")
            print(f"wall stopped steps: {int(np.sum(r['wall_stopped_steps']))}")
        print(f"minimum wall clearance: {float(np.nanmin(clear)) if np.any(~np.isnan(clear)) else float('nan')}")
    if teams is not None and team_solid:
        print(f"team blocked rate: {float(np.mean(r['team_blocked_steps'] > 0))}")
        print(f"team stopped steps: {int(np.sum(r['team_stopped_steps']))}")
        print(f"team inside steps: {int(np.sum(r['team_inside_steps']))}")
    if check_spec:
        worst = int(np.argmin(r["robustness"]))
        print(f"specification satisfied: {int(np.sum(r['satisfied']))} of {len(r['satisfied'])} robots")
        print(f"worst robustness: {float(r['robustness'][worst])} (robot {worst}, clause {int(r['weakest'][worst])})")
        if shared:                                         # the team's verdict: a station someone visited is visited
            from mobrob_amd.waypoints import spec_team_result
            team = spec_team_result(r, monitored["spec"], shared["share"])
            worst = int(np.argmin(team["team_robustness"]))
            print(f"team specification satisfied: {int(np.sum(team['team_satisfied']))} of {len(team['team_satisfied'])} teams")
            print(f"worst team robustness: {float(team['team_robustness'][worst])} (team {worst}, clause {int(team['team_weakest'][worst])}, "
                  f"member {int(team['team_member'][worst, team['team_weakest'][worst]])})")
        r.update(team if shared else {})
    return r


def make_schedule(release, stagger, n, K, team_size=None):
    """--release / --stagger -> a Schedule, or None without either: release [K] or [n][K] (None: zeros) plus m * stagger for
    robot m of its team (robot i without teams)"""
    from mobrob_amd.envs.goal_rules import Schedule
    if release is None and not stagger:
        return None
    if int(stagger) < 0:
        raise ValueError("--stagger must be >= 0")
    rel = np.zeros((n, K), np.int64) if release is None else np.asarray(release)
    if not np.issubdtype(rel.dtype, np.integer):
        raise ValueError("--release must hold integers")
    rel = np.broadcast_to(rel, (n, rel.shape[-1])) if rel.ndim == 1 else rel
    member = np.arange(n) % int(team_size) if team_size else np.arange(n)
    return Schedule(rel + int(stagger) * member[:, None])


def report_hazards(r):
    """The three hazard lines: mean cost per robot, violation rate (robots with a step of cost > 0), minimum clearance."""
    print(f"mean hazard cost: {float(np.mean(r['cost_sum']))}")
    print(f"violation rate: {float(np.mean(r['violation_steps'] > 0))}")
    print(f"minimum clearance: {float(np.nanmin(r['min_clearance'])) if np.any(r['steps'] > 0) else float('nan')}")


def report_teams(r):
    """The three team lines: mean separation cost per robot, conflict rate (robots with a step of cost > 0), minimum clearance
    to a team-mate."""
    clear = r["min_team_clearance"]
    print(f"mean team cost: {float(np.mean(r['team_cost_sum']))}")
    print(f"conflict rate: {float(np.mean(r['conflict_steps'] > 0))}")
    print(f"minimum team clearance: {float(np.nanmin(clear)) if np.any(~np.isnan(clear)) else float('nan')}")


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env-name", type=str, default="point")
    ap.add_argument("--policy-name", type=str, default="ppo")
    ap.add_argument("--waypoints", type=str, default=None, help="[K][P] or [n][K][P] positions (.npy)")
    ap.add_argument("--goal", type=str, default=None, help="x,y (x,y,z): plan the waypoints to this goal instead of --waypoints")
    ap.add_argument("--goals", type=str, default=None, help="[team size][P] or [n][P] places (.npy): plan robot i to goals[i] instead of --goal")
    ap.add_argument("--assign", type=str, default=None, choices=("sum", "makespan"),
                    help="with --goals and --team-size: assign the places inside every team at least total (or least largest) path cost")
    ap.add_argument("--plan-cells", type=int, default=64, help="grid cells a side of the planner (32, 64, 128)")
    ap.add_argument("--plan-smooth", action="store_true", default=False, help="smooth the planned paths by line of sight")
    ap.add_argument("--plan-time-smooth", action="store_true", default=False,
                    help="with --goal and --hazard-frames or --team-size: smooth the time plan, every leg tested in every layer it spans")
    ap.add_argument("--plan-max-leg", type=int, default=None,
                    help="with --plan-time-smooth and --team-size: the actions of a smoothed leg at most (default 8; 0: no cap)")
    ap.add_argument("--plan-los-margin", type=int, default=1, choices=(0, 1), help="cells a smoothed leg keeps clear on either side")
    ap.add_argument("--plan-clearance", type=str, default=None,
                    help="REACH,WEIGHT (1 .. 8, 1 .. 16): a static plan that pays WEIGHT a cell of missing clearance within REACH cells of obstacles")
    ap.add_argument("--plan-layer-steps", type=int, default=10, help="with --hazard-frames or --team-size: steps a robot is given for one move or wait")
    ap.add_argument("--plan-reserve", type=int, default=None,
                    help="with --goal and --team-size: cells a mate's planned walk reserves around itself, 0 .. 4 (default: ceil(separation / cell))")
    ap.add_argument("--plan-retries", type=int, default=0,
                    help="with --goal and --team-size: reordering rounds of a team plan, 0 .. 8: a team with parked members plans again, those first")
    ap.add_argument("--plan-layers", type=int, default=64, help="with --hazard-frames or --team-size: actions planned in time before the tail (1 .. 256)")
    ap.add_argument("--robots", type=int, default=1)
    ap.add_argument("--max-steps", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--host", action="store_true", default=False, help="the Python loop over get_env instead of one device call")
    ap.add_argument("--hazards", type=str, default=None, help="[M][2] hazard centres (.npy): report hazard costs")
    ap.add_argument("--hazard-size", type=float, default=0.3, help="hazard radius (hazards_size)")
    ap.add_argument("--hazard-frames", type=str, default=None, help="[F][M][3] x, y, radius per frame (.npy): moving hazards")
    ap.add_argument("--frame-steps", type=int, default=1, help="steps per hazard frame")
    ap.add_argument("--hazard-loop", action="store_true", default=False, help="start over after the last frame (else hold it)")
    ap.add_argument("--horizon", type=int, default=None, help="run as a chain of calls of this many steps (a planner's rounds)")
    ap.add_argument("--leg-steps", type=int, default=0, help="step budget per waypoint; a robot that spends it stalls (0: none)")
    ap.add_argument("--team-size", type=int, default=None, help="teams of this many consecutive robots (1, 2, 4, 8, 16): report separation costs")
    ap.add_argument("--separation", type=float, default=0.3, help="distance team-mates must keep")
    ap.add_argument("--release", type=str, default=None, help="[K] or [n][K] release steps of the waypoints (.npy, integers)")
    ap.add_argument("--walls", type=str, default=None, help="[M][4] boxes cx, cy, hx, hy (.npy): report wall contacts and crossings")
    ap.add_argument("--team-solid", action="store_true", default=False,
                    help="with --team-size: team-mates block each other (stop and slide at the square of half-width --separation "
                         "around a mate); alone or with --solid walls, not with hazards, not with --host")
    ap.add_argument("--solid", action="store_true", default=False, help="with --walls / --arena: the walls block (robots stop and slide)")
    ap.add_argument("--arena", action="store_true", default=False, help="add the reference's turtlebot3 enclosure to the walls")
    ap.add_argument("--robot-radius", type=float, default=0.1, help="the robot's footprint for wall contact")
    ap.add_argument("--stagger", type=int, default=0, help="release robot m of a team (robot i without teams) m * S steps later")
    ap.add_argument("--check-spec", action="store_true", default=False,
                    help="with --goal: monitor 'eventually inside the reach radius around the goal' and, with --walls / --arena, "
                         "'always outside every wall'; with --hazard-frames, 'outside every moving hazard from the first step on'; "
                         "with --team-size / --separation, 'always further than the separation from every team-mate'; report the "
                         "satisfied robots and the worst robustness")
    ap.add_argument("--spec-hold", type=int, default=0,
                    help="with --check-spec: 'inside the reach radius around the goal for H consecutive steps' (0 .. 255) in place of "
                         "'eventually inside'; 0: eventually inside")
    ap.add_argument("--plan-spec", action="store_true", default=False,
                    help="with --check-spec: plan the specification's stations (here: the reach circle around --goal, the walls as keep-out "
                         "regions) with GridPlanner.plan_spec instead of planning to --goal, follow with the plan's schedule, then monitor")
    ap.add_argument("--pace", type=int, default=None,
                    help="with --plan-spec: the steps a robot is given for one orthogonal move (required with --spec-hold)")
    ap.add_argument("--replan-spec", action="store_true", default=False,
                    help="with --plan-spec: between the calls of the run (--horizon, --leg-steps) plan a stalled robot again from where it "
                         "stands, for the stations not yet visited (GridPlanner.spec_callback)")
    ap.add_argument("--partial", action="store_true", default=False,
                    help="with --plan-spec: a robot that cannot keep every window keeps the stations it still can (plan_spec(partial=True))")
    ap.add_argument("--share", type=int, default=None,
                    help="with --plan-spec: share the stations within teams of N consecutive robots, each station to one member "
                         "(plan_spec(share=N)); prints the team verdict (waypoints.spec_team_result)")
    ap.add_argument("--share-objective", choices=("makespan", "sum"), default=None,
                    help="with --share: the team done as early as possible (makespan, the default) or with the least total (sum)")
    ap.add_argument("--tile256", action="store_true", default=False,
                    help="a 2x256 tanh policy: run calls without hazards, teams or walls as one launch (PPOEngine.set_eval_tile256)")
    ap.add_argument("--tile256-wide", action="store_true", default=False,
                    help="... and calls WITH hazards as well (PPOEngine.set_eval_tile256_wide); implies --tile256; walls and teams stay per step")
    return ap


if __name__ == "__main__":
    ap = build_parser()
    args = ap.parse_args()
    if args.goals is not None and (args.goal is not None or args.waypoints is not None):
        ap.error("--goals excludes --goal and --waypoints")
    if args.assign is not None and (args.goals is None or args.team_size is None):
        ap.error("--assign needs --goals and --team-size")
    if args.goals is None and (args.waypoints is None) == (args.goal is None):
        ap.error("give --waypoints or --goal, not both")
    if args.check_spec and args.goal is None:
        ap.error("--check-spec needs --goal")
    if args.spec_hold != 0 and not args.check_spec:
        ap.error("--spec-hold needs --check-spec")
    if args.plan_spec and not args.check_spec:
        ap.error("--plan-spec needs --check-spec")
    if args.pace is not None and not args.plan_spec:
        ap.error("--pace needs --plan-spec")
    if (args.replan_spec or args.partial) and not args.plan_spec:
        ap.error("--replan-spec and --partial need --plan-spec")
    if args.share is not None and (not args.plan_spec or args.team_size is not None):
        ap.error("--share needs --plan-spec and excludes --team-size")
    if args.share_objective is not None and args.share is None:
        ap.error("--share-objective needs --share")
    try:
        check_chain(args.max_steps, args.horizon, args.leg_steps)
    except ValueError as ex:
        ap.error(str(ex))
    follow(args.env_name, args.policy_name, None if args.waypoints is None else np.load(args.waypoints), args.robots, args.max_steps, args.host, args.seed,
           hazards=None if args.hazards is None else (np.load(args.hazards), args.hazard_size), horizon=args.horizon,
           leg_steps=args.leg_steps, hazard_frames=None if args.hazard_frames is None else np.load(args.hazard_frames),
           frame_steps=args.frame_steps, hazard_loop=args.hazard_loop, team_size=args.team_size, separation=args.separation,
           release=None if args.release is None else np.load(args.release), stagger=args.stagger,
           walls=None if args.walls is None else np.load(args.walls), arena=args.arena, robot_radius=args.robot_radius,
           goal=None if args.goal is None else [float(v) for v in args.goal.split(",")], plan_cells=args.plan_cells,
           plan_smooth=args.plan_smooth, plan_los_margin=args.plan_los_margin, plan_layer_steps=args.plan_layer_steps,
           plan_layers=args.plan_layers, plan_reserve=args.plan_reserve, plan_time_smooth=args.plan_time_smooth, plan_max_leg=args.plan_max_leg,
           plan_retries=args.plan_retries, goals=None if args.goals is None else np.load(args.goals), assign=args.assign,
           plan_clearance=None if args.plan_clearance is None else [int(v) for v in args.plan_clearance.split(",")], solid=args.solid,
           tile256=args.tile256 or args.tile256_wide, tile256_wide=args.tile256_wide, team_solid=args.team_solid,
           check_spec=args.check_spec, spec_hold=args.spec_hold, plan_spec=args.plan_spec, pace=args.pace,
           replan_spec=args.replan_spec, partial=args.partial, share=args.share, share_objective=args.share_objective)
