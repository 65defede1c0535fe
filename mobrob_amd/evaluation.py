"""`evaluate_policy` with the signature and return values of stable-baselines3 2.0 (sb3 common/evaluation.py).

Two paths:
  * device: `env` is a `DeviceGoalVecEnv` -- the whole evaluation is ONE engine call (mobrob_ppo_evaluate_goal_env): fresh
    robots, deterministic or sampled actions, SB3's per-environment episode quota (n_eval_episodes + i) // n_envs, float64
    returns.  Episodes are listed robot by robot (SB3 lists them in the order they finish; means and stds are the same).
  * host: any other VecEnv (`HostVecEnv`, `make_vec_env(get_env, ...)`) or a single gymnasium-style env -- SB3's loop over
    `model.predict`, one batched call per step.  No native code of its own.
"""
from __future__ import annotations

import warnings

import numpy as np


def _engine_of(model):
    return getattr(model, "engine", model)


def _device_episodes(model, env, n_eval_episodes, deterministic, seed=None):
    """(returns, lengths, successes) of the device path, quota split as SB3's episode_count_targets."""
    n = int(env.num_envs)
    quota = np.array([(n_eval_episodes + i) // n for i in range(n)], np.int32)
    r = env.evaluate(_engine_of(model), episodes=n_eval_episodes, quota=quota, deterministic=deterministic, seed=seed)
    keep = ~np.isnan(r["episode_returns"])
    return (list(r["episode_returns"][keep].astype(float)), list(r["episode_lengths"][keep].astype(int)),
            list(r["episode_success"][keep].astype(bool)))


class _SingleEnv:
    """A gymnasium-style env behind the VecEnv protocol for one environment (SB3 wraps it in a DummyVecEnv)."""

    def __init__(self, env):
        self.env, self.num_envs = env, 1

    def reset(self):
        obs, _ = self.env.reset()
        return np.asarray(obs, np.float32)[None]

    def step(self, actions):
        o, r, term, trunc, info = self.env.step(actions[0])
        info = dict(info)
        done = bool(term or trunc)
        info["TimeLimit.truncated"] = bool(trunc and not term)
        if done:
            info["terminal_observation"] = np.asarray(o, np.float32)
            o, _ = self.env.reset()
        return np.asarray(o, np.float32)[None], np.array([r], np.float32), np.array([done]), [info]


def _host_episodes(model, env, n_eval_episodes, deterministic, render=False, callback=None):
    """SB3 evaluate_policy's loop (episode_count_targets, current_rewards in float64)."""
    if not hasattr(env, "num_envs"):
        env = _SingleEnv(env)
    n_envs = int(env.num_envs)
    episode_rewards, episode_lengths, successes = [], [], []
    episode_counts = np.zeros(n_envs, dtype="int")
    episode_count_targets = np.array([(n_eval_episodes + i) // n_envs for i in range(n_envs)], dtype="int")
    current_rewards = np.zeros(n_envs)
    current_lengths = np.zeros(n_envs, dtype="int")
    observations = env.reset()
    states = None
    episode_starts = np.ones((n_envs,), dtype=bool)
    while (episode_counts < episode_count_targets).any():
        actions, states = model.predict(observations, state=states, episode_start=episode_starts, deterministic=deterministic)
        new_observations, rewards, dones, infos = env.step(actions)
        current_rewards += rewards
        current_lengths += 1
        for i in range(n_envs):
            if episode_counts[i] < episode_count_targets[i]:
                reward, done, info = rewards[i], dones[i], infos[i]
                episode_starts[i] = done
                if callback is not None:
                    callback(locals(), globals())
                if dones[i]:
                    episode_rewards.append(float(current_rewards[i]))
                    episode_lengths.append(int(current_lengths[i]))
                    successes.append(bool(info.get("is_success", not info.get("TimeLimit.truncated", False))))
                    episode_counts[i] += 1
                    current_rewards[i] = 0
                    current_lengths[i] = 0
        observations = new_observations
        if render and hasattr(env, "render"):
            env.render()
    return episode_rewards, episode_lengths, successes


def evaluate_episodes(model, env, n_eval_episodes=10, deterministic=True, render=False, callback=None, seed=None):
    """(episode returns, lengths, successes) -- the lists evaluate_policy and EvalCallback are built on."""
    from .envs.vec_env import DeviceGoalVecEnv
    if isinstance(env, DeviceGoalVecEnv):
        return _device_episodes(model, env, int(n_eval_episodes), deterministic, seed=seed)
    return _host_episodes(model, env, int(n_eval_episodes), deterministic, render=render, callback=callback)


def evaluate_policy(model, env, n_eval_episodes=10, deterministic=True, render=False, callback=None, reward_threshold=None,
                    return_episode_rewards=False, warn=True):
    """Runs the policy for `n_eval_episodes` episodes and returns (mean reward, std of reward) -- or, with
    return_episode_rewards=True, the lists of per-episode rewards and lengths.  `model` is a PPO (or anything with
    `predict`; the device path needs its `engine`).  `callback(locals, globals)` is called after every step of the host
    path (the device path runs in one launch and has no per-step hook: a callback is refused there)."""
    from .envs.vec_env import DeviceGoalVecEnv
    if isinstance(env, DeviceGoalVecEnv) and callback is not None:
        raise ValueError("evaluate_policy: a per-step callback needs a host environment (the device evaluation is one launch)")
    if warn and render and isinstance(env, DeviceGoalVecEnv):
        warnings.warn("render is not supported for the device goal environment; ignored", UserWarning)
    episode_rewards, episode_lengths, _ = evaluate_episodes(model, env, n_eval_episodes, deterministic, render, callback)
    mean_reward = np.mean(episode_rewards)
    std_reward = np.std(episode_rewards)
    if reward_threshold is not None:
        assert mean_reward > reward_threshold, "Mean reward below threshold: " f"{mean_reward:.2f} < {reward_threshold:.2f}"
    if return_episode_rewards:
        return episode_rewards, episode_lengths
    return mean_reward, std_reward
