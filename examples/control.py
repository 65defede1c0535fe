#!/usr/bin/env python3
"""Run a trained policy in its environment and report the reward it collects.

Same protocol and command line as the reference script (/root/reference/examples/control.py:11-82), so that numbers
from the two are comparable (last row):

* `--epochs` evaluation epochs (default 5) of exactly STEPS_PER_EPOCH = 1000 environment steps each (:36-39);
* the policy acts deterministically, `policy.predict(obs, deterministic=True)` (:40);
* reaching the goal (`terminated`) RESETS the environment and the epoch goes on -- the epoch's figure is the reward
  accumulated over all 1000 steps, usually several episodes, not the return of one episode (:41-46);
* three report lines: `average reward`, `reward stds`, `rewards` (:61-63);
* defaults `--env-name point --policy-name ppo` (:68-69).

`--robots N` runs the same protocol for max(N, epochs) robots at once on the device goal environment (the kinematic
stand-in stepped by the engine, no time limit, reset on goal): ONE engine call instead of one `predict` round trip per robot
and step.  Each robot is one epoch: the `rewards` line lists max(N, epochs) figures.  Without `--robots` the script runs the
host loop above, exactly as before.  With `--robots`, `--hazards FILE.npy` ([M][2] hazard centres, radius 0.3, the reference
Engine's shaped hazard cost) adds three lines: the mean cost per robot, the violation rate and the minimum clearance.

GUI rendering, the 5 ms sleep that paces the Bullet GUI and video recording (:24-33, :48-52) need the real MuJoCo / Bullet
simulators; the kinematic stand-in robots have nothing to draw, so `--no-gui` / `--video-path` are accepted and ignored.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STEPS_PER_EPOCH = 1000


def evaluation_epoch(env, policy, steps=STEPS_PER_EPOCH):
    """Reward collected over `steps` consecutive environment steps, restarting the episode whenever the goal is reached."""
    collected = 0.0
    obs, _ = env.reset()
    for _ in range(steps):
        action, _state = policy.predict(obs, deterministic=True)
        obs, reward, terminated, _truncated, _info = env.step(action)
        if terminated:
            obs, _ = env.reset()
        collected += reward
    return collected


def simulate(env_name, policy_name="ppo", epochs=5, no_gui=True, video_path=None, env=None, policy=None):
    """env / policy: injected instances (tests); by default `get_env(env_name, terminate_on_goal=True)` and the
    checkpoint `data/policies/<env_name>-<policy_name>.zip`, exactly what the reference script builds (:19-20)."""
    if env is None or policy is None:
        from mobrob_amd import get_env, load_policy
        env = get_env(env_name, enable_gui=not no_gui, terminate_on_goal=True) if env is None else env
        policy = load_policy(env_name, policy_name) if policy is None else policy
    rewards = [evaluation_epoch(env, policy) for _ in range(epochs)]
    print(f"average reward: {np.mean(rewards)}")
    print(f"reward stds: {np.std(rewards)}")
    print(f"rewards: {rewards}")
    return rewards


def simulate_device(env_name, policy_name="ppo", epochs=5, robots=1, policy=None, seed=0, hazards=None, tile256=False, tile256_wide=False):
    """The protocol of `simulate` for max(robots, epochs) robots in one device evaluation (PPOEngine.evaluate_goal_env)."""
    from mobrob_amd import load_policy
    from mobrob_amd.envs.vec_env import DeviceGoalVecEnv
    policy = load_policy(env_name, policy_name) if policy is None else policy
    if tile256 or tile256_wide:   # a 2x256 tanh policy: the evaluation (without hazards) as one launch; ValueError on any other policy
        policy.engine.set_eval_tile256(True)
    if tile256_wide:   # ... and with --hazards too (implies tile256)
        policy.engine.set_eval_tile256_wide(True)
    n = max(int(robots), int(epochs))
    env = DeviceGoalVecEnv.for_robot(env_name, n, time_limit=0, seed=seed, terminate_on_goal=True)
    from mobrob_amd.envs.goal_rules import Hazards
    hz = None if hazards is None else Hazards(hazards, indicator=False)
    r = env.evaluate(policy.engine, n_robots=n, max_steps=STEPS_PER_EPOCH, episodes=0, deterministic=True, hazards=hz)
    rewards = [float(x) for x in r["reward_sum"]]
    print(f"average reward: {np.mean(rewards)}")
    print(f"reward stds: {np.std(rewards)}")
    print(f"rewards: {rewards}")
    if hz is not None:
        print(f"mean hazard cost: {float(np.mean(r['cost_sum']))}")
        print(f"violation rate: {float(np.mean(r['violation_steps'] > 0))}")
        print(f"minimum clearance: {float(np.min(r['min_clearance']))}")
    return rewards


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env-name", type=str, default="point")
    ap.add_argument("--policy-name", type=str, default="ppo")
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--no-gui", action="store_true", default=False)
    ap.add_argument("--video-path", type=str, default=None)
    ap.add_argument("--robots", type=int, default=None,
                    help="evaluate max(ROBOTS, epochs) robots at once on the device (one engine call)")
    ap.add_argument("--hazards", type=str, default=None, help="[M][2] hazard centres (.npy), with --robots: report hazard costs")
    ap.add_argument("--tile256", action="store_true", default=False,
                    help="with --robots, a 2x256 tanh policy: the evaluation as one launch (PPOEngine.set_eval_tile256)")
    ap.add_argument("--tile256-wide", action="store_true", default=False,
                    help="... and the evaluation with --hazards as well (PPOEngine.set_eval_tile256_wide); implies --tile256")
    return ap


if __name__ == "__main__":
    ap = build_parser()
    a = ap.parse_args()
    if a.hazards is not None and a.robots is None:
        ap.error("--hazards needs --robots (the device evaluation)")
    if (a.tile256 or a.tile256_wide) and a.robots is None:
        ap.error("--tile256 / --tile256-wide need --robots (the device evaluation)")
    if a.robots is not None:
        simulate_device(env_name=a.env_name, policy_name=a.policy_name, epochs=a.epochs, robots=a.robots,
                        hazards=None if a.hazards is None else np.load(a.hazards), tile256=a.tile256 or a.tile256_wide,
                        tile256_wide=a.tile256_wide)
        sys.exit(0)
    simulate(env_name=a.env_name, policy_name=a.policy_name, epochs=a.epochs, no_gui=a.no_gui, video_path=a.video_path)
