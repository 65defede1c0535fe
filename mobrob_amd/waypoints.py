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


def _host_follow(model, make_env, start, wp, nw, max_steps, deterministic, seed, path_stride, hazards=None):
    """The semantics, one robot after another on EnvWrapper's public API (make_env(i) -> the robot's env)."""
    from .envs.goal_rules import hazard_cost
    n, K, P = wp.shape
    if hazards is not None:
        hazards.check_robots(n)
    cost_sum, viol = np.zeros(n), np.zeros(n, np.int64)
    first, min_clear = np.full(n, -1, np.int64), np.full(n, np.nan)
    arrival = np.full((n, K), -1, np.int64)
    reached, steps = np.zeros(n, np.int64), np.zeros(n, np.int64)
    reward_sum, final_distance = np.zeros(n), np.full(n, np.nan)
    path = np.zeros((max_steps // path_stride + 1, n, P), np.float32) if path_stride > 0 else None
    for i in range(n):
        pos = start[i].astype(np.float64)
        if path is not None:
            path[0, i] = pos
        if nw[i] > 0:
            env = make_env(i)
            if hazards is not None:
                rows = hazards.rows(i)
                env.set_hazards(rows[:, :2], rows[:, 2], hazards.cost, hazards.indicator)
                min_clear[i] = np.inf
            if seed is not None:
                env.seed(int(seed) + i)
            env.env.reset()                            # the simulator at rest: every robot starts with zero velocity
            obs, _ = env.reset(init_pos=start[i])
            env.set_goal(wp[i, 0])
            obs = env.get_obs()
            k = 0
            for t in range(max_steps):
                a, _ = model.predict(obs, deterministic=deterministic)
                obs, r, _, _, info = env.step(a)
                reward_sum[i] += float(r)
                steps[i] = t + 1
                pos = np.asarray(env.get_pos(), np.float64)[:P]
                if hazards is not None:
                    cost_sum[i] += info["cost"]
                    if info["cost"] > 0:
                        viol[i] += 1
                        first[i] = t + 1 if first[i] < 0 else first[i]
                    min_clear[i] = min(min_clear[i], hazard_cost(pos, rows)[1])
                if path is not None and (t + 1) % path_stride == 0:
                    path[(t + 1) // path_stride, i] = pos
                if env.reached():
                    arrival[i, k] = t + 1
                    k += 1
                    if k == nw[i]:
                        break
                    env.set_goal(wp[i, k])
                    obs = env.get_obs()
            reached[i] = k
            final_distance[i] = float(np.linalg.norm(np.asarray(env.get_goal(), np.float64)[:P] - pos))
            if hazards is not None:
                env.set_hazards(None)
        if path is not None:
            path[steps[i] // path_stride + 1:, i] = pos
    out = {"arrival": arrival, "reached": reached, "steps": steps, "reward_sum": reward_sum, "final_distance": final_distance,
           "trace": None, "persistent": None}
    if hazards is not None:
        out.update({"cost_sum": cost_sum, "violation_steps": viol, "first_violation": first, "min_clearance": min_clear})
    if path is not None:
        out["path"] = path
    return out


def follow_waypoints(model, env, start, waypoints, n_waypoints=None, *, max_steps=1000, deterministic=True, seed=0,
                     path_stride=0, hazards=None):
    """Every robot i follows waypoints[i][:n_waypoints[i]] from start[i] under `model` (a PPO, or for the host path anything
    with `.predict`).  `env`: a DeviceGoalVecEnv (device path), an EnvWrapper, or an env name for `get_env` (host path; a
    fresh environment per robot for a name, the given one reused robot after robot otherwise).  Returns the dict described in
    the module docstring.  hazards: a goal_rules.Hazards (hazard costs, see the module docstring)."""
    from .envs.vec_env import DeviceGoalVecEnv
    from .envs.wrapper import EnvWrapper, TimeLimit, get_env
    max_steps, path_stride = int(max_steps), int(path_stride)
    if max_steps < 1 or path_stride < 0:
        raise ValueError("max_steps must be >= 1 and path_stride >= 0")
    if isinstance(env, DeviceGoalVecEnv):
        return env.follow(getattr(model, "engine", model), start, waypoints, n_waypoints, max_steps=max_steps,
                          deterministic=deterministic, seed=seed, path_stride=path_stride, hazards=hazards)
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
    s, wp, nw = follow_inputs(start, waypoints, n_waypoints, pos_dim)
    return _host_follow(model, make_env, s, wp, nw, max_steps, deterministic, seed, path_stride, hazards)
